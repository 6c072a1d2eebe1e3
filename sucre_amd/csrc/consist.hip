// Cross-view colour consistency of restored images for gfx950 (sucre_view_consistency; the description: consist.h).
#include "consist.h"
#include "fit_math.h"
#include "handoff.h"
#include "match_pixel.h"

namespace sucre {

struct ConsistArgs {
    const float *depth1;             // target: (H,W) depth map
    const uint8_t *rgb1;             //         (H,W,3) uint8 colours, nullable
    const float *J1;                 //         (H,W,3) restored image
    const sucre_view_t *views;       // [n_views], plain form
    const float *const *J_views;     // [n_views] device pointers, NULL = the view takes no part
    int n_views, tiles_x, n_tiles, tiles_per_xcd;
    int32_t *count;                  // (H,W)
    float *ssd;                      // (H,W,3)
    uint32_t *tv_counts;             // scratch [n_views][n_tiles][4 waves]: matches | valid pairs << 16
    float *tv_sums;                  // scratch [n_views][n_tiles][4 waves][24], written where the wave has a valid pair in the view
    double *stats;                   // (n_views, 26)
};

// The view table and the pointer array are kernel parameters of their own, __restrict__: only then may the compiler read them
// with scalar loads (through the by-value struct every field of a view came by a vector load of its own, each waited for: 2.8 ms
// per 1080p target against 64 views).
__global__ __launch_bounds__(256) void consistency_kernel(const CamDev c1, const ConsistArgs A, const sucre_view_t *__restrict__ views,
                                                          const float *const *__restrict__ J_views, const float *__restrict__ depth1,
                                                          const uint8_t *__restrict__ rgb1, const float *__restrict__ J1,
                                                          int32_t *__restrict__ count, float *__restrict__ ssd_out,
                                                          uint32_t *__restrict__ tv_counts, float *__restrict__ tv_sums) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // workgroups are dealt round-robin over the 8 XCDs: every XCD gets one contiguous band of tiles, so that the gathers of
    // neighbouring tiles share that XCD's L2 (as match_kernel; speed only)
    const int tile = (blockIdx.x & 7) * A.tiles_per_xcd + (blockIdx.x >> 3);
    if (tile >= A.n_tiles) return;   // (no barrier below: every wave is on its own)
    const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
    const int u1 = tx * kTile + (lane & 15);
    const int v1 = ty * kTile + 4 * wave + (lane >> 4);
    const float W1f = (float)c1.W, H1f = (float)c1.H;
    const bool pin1 = pinhole_form(c1.K) && pinhole_form(c1.Kinv);
    const bool inside = v1 < c1.H && u1 < c1.W;
    const size_t o = (size_t)v1 * c1.W + u1;

    float d1 = 0.0f, a[3] = {0.0f, 0.0f, 0.0f};
    uint32_t ka = 0u;   // the target's raw colour, r | g << 8 | b << 16
    if (inside) {
        d1 = depth1[o];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = J1[o * 3 + c];
        if (rgb1) ka = (uint32_t)rgb1[o * 3] | ((uint32_t)rgb1[o * 3 + 1] << 8) | ((uint32_t)rgb1[o * 3 + 2] << 16);
    }
    const bool ok1 = d1 > 0.0f;
    const bool a_ok = inside && a[0] == a[0] && a[1] == a[1] && a[2] == a[2];
    const float ra[3] = {unit_from_u8(ka & 255u), unit_from_u8((ka >> 8) & 255u), unit_from_u8((ka >> 16) & 255u)};
    float wP[3];
    {
        float cP[3];
        unproject(c1.Kinv, pin1, (float)u1, (float)v1, d1, cP);
        rigid(c1.R, c1.t, cP, wP);
    }
    int cnt = 0;
    float ssd[3] = {0.0f, 0.0f, 0.0f};

    for (int k = 0; k < A.n_views; ++k) {
        const float *__restrict__ Jk = J_views[k];   // wave-uniform: scalar loads
        if (Jk == nullptr) continue;                   // the view takes no part; the second kernel zeroes its row
        const sucre_view_t *vw = views + k;
        const uint8_t *__restrict__ rgb2 = vw->rgb;
        const bool raw = rgb1 != nullptr && rgb2 != nullptr;
        const bool pin = pin1 && pinhole_form(vw->K) && pinhole_form(vw->Kinv);
        bool m = ok1;
        size_t q = 0;
        if (m) {
            float c2[3];
            uint32_t unused;
            m = match_pixel(c1, W1f, H1f, vw, false, (float)vw->W, (float)vw->H, pin, wP, u1, v1, &q, c2, &unused);
        }
        bool valid = false;
        float b[3] = {0.0f, 0.0f, 0.0f};
        uint32_t kb = 0u;
        if (m) {   // q lies inside view k (project()'s bound test against the view's own W and H)
            const auto *pb = global_ptr(Jk) + q * 3;
            b[0] = pb[0]; b[1] = pb[1]; b[2] = pb[2];
            valid = a_ok && b[0] == b[0] && b[1] == b[1] && b[2] == b[2];
            if (raw) {
                const auto *pc = global_ptr(rgb2) + q * 3;
                kb = (uint32_t)pc[0] | ((uint32_t)pc[1] << 8) | ((uint32_t)pc[2] << 16);
            }
        }
        const int n_match = __builtin_popcountll(__ballot(m)), n_valid = __builtin_popcountll(__ballot(valid));
        const size_t tv = ((size_t)k * A.n_tiles + tile) * 4 + wave;
        if (lane == 0) tv_counts[tv] = (uint32_t)n_match | ((uint32_t)n_valid << 16);
        if (n_valid == 0) continue;   // wave-uniform; most (tile, view) pairs of a survey stop here
        float s[kConsistSums];
#pragma unroll
        for (int c = 0; c < 3; ++c) {   // (selects, not branches: an invalid pair adds exact zeros)
            const float av = valid ? a[c] : 0.0f, bv = valid ? b[c] : 0.0f, d = av - bv;
            ssd[c] = __builtin_fmaf(d, d, ssd[c]);
            s[c] = d * d; s[3 + c] = av * av; s[6 + c] = bv * bv; s[9 + c] = av * bv;
            const float rav = valid && raw ? ra[c] : 0.0f, rbv = valid && raw ? unit_from_u8((kb >> (8 * c)) & 255u) : 0.0f, rd = rav - rbv;
            s[12 + c] = rd * rd; s[15 + c] = rav * rav; s[18 + c] = rbv * rbv; s[21 + c] = rav * rbv;
        }
        cnt += valid ? 1 : 0;
#pragma unroll
        for (int i = 0; i < kConsistSums; ++i) s[i] = wave_sum_lane0(s[i]);
        if (lane == 0) {
            float4 *out = reinterpret_cast<float4 *>(tv_sums + tv * kConsistSums);
#pragma unroll
            for (int i = 0; i < kConsistSums / 4; ++i) out[i] = make_float4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
        }
    }

    if (inside) {
        count[o] = cnt;
#pragma unroll
        for (int c = 0; c < 3; ++c) ssd_out[o * 3 + c] = ssd[c];
    }
}

// view k's row.  A tile's sums: its four waves' (four rows of the tile each), added in float32 in wave order -- the float32 sum of
// the (16x16 tile, view) pair; the tiles then in float64 in a fixed order (thread t takes tiles t, t + 256, ...; a fixed-shape
// tree; the four waves in order), as residual_view_sum_kernel.  The count words say which sums were written.  One workgroup per view.
__global__ __launch_bounds__(256) void consistency_view_sum_kernel(const ConsistArgs A) {
    __shared__ double w4[kConsistStats][4];
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double x[kConsistStats];
#pragma unroll
    for (int i = 0; i < kConsistStats; ++i) x[i] = 0.0;
    if (A.J_views[k] != nullptr) {   // (workgroup-uniform)
        for (int tile = t; tile < A.n_tiles; tile += 256) {
            const size_t tv = ((size_t)k * A.n_tiles + tile) * 4;
            const uint4 c4 = *reinterpret_cast<const uint4 *>(A.tv_counts + tv);
            const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
            float f[kConsistSums];
#pragma unroll
            for (int i = 0; i < kConsistSums; ++i) f[i] = 0.0f;
            uint32_t matches = 0u, pairs = 0u;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                matches += c[w] & 0xffffu;
                pairs += c[w] >> 16;
                if ((c[w] >> 16) == 0u) continue;
                const float4 *p = reinterpret_cast<const float4 *>(A.tv_sums + (tv + w) * kConsistSums);
#pragma unroll
                for (int i = 0; i < kConsistSums / 4; ++i) {
                    const float4 q = p[i];
                    f[4 * i] += q.x; f[4 * i + 1] += q.y; f[4 * i + 2] += q.z; f[4 * i + 3] += q.w;
                }
            }
            x[0] += (double)matches;
            x[1] += (double)pairs;
#pragma unroll
            for (int i = 0; i < kConsistSums; ++i) x[2 + i] += (double)f[i];
        }
    }
#pragma unroll
    for (int i = 0; i < kConsistStats; ++i) {
        const double y = wave_sum_lane0(x[i]);
        if (lane == 0) w4[i][wave] = y;
    }
    __syncthreads();
    if (t < kConsistStats) A.stats[(size_t)k * kConsistStats + t] = ((w4[t][0] + w4[t][1]) + w4[t][2]) + w4[t][3];
}

hipError_t launch_consistency(int H, int W, int n_views, const sucre_view_t &target, const sucre_view_t *views_dev, const float *J_target,
                              const float *const *J_views, int32_t *count, float *ssd, double *stats, void *scratch, hipStream_t s) {
    ConsistArgs A = {};
    A.depth1 = target.depth; A.rgb1 = target.rgb; A.J1 = J_target;
    A.views = views_dev; A.J_views = J_views;
    A.n_views = n_views;
    A.tiles_x = (W + kTile - 1) / kTile;
    A.n_tiles = A.tiles_x * ((H + kTile - 1) / kTile);
    A.tiles_per_xcd = (A.n_tiles + 7) / 8;
    A.count = count; A.ssd = ssd; A.stats = stats;
    A.tv_counts = static_cast<uint32_t *>(scratch);
    A.tv_sums = reinterpret_cast<float *>(static_cast<uint8_t *>(scratch) + consist_counts_bytes(A.n_tiles, n_views));
    hipLaunchKernelGGL(consistency_kernel, dim3(8 * A.tiles_per_xcd), dim3(256), 0, s, to_cam(target), A, A.views, A.J_views, A.depth1, A.rgb1,
                       A.J1, A.count, A.ssd, A.tv_counts, A.tv_sums);
    hipLaunchKernelGGL(consistency_view_sum_kernel, dim3(n_views), dim3(256), 0, s, A);
    return hipGetLastError();
}

}  // namespace sucre
