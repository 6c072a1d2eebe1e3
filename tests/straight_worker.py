"""Child process of tests/test_gpu_straight_chunks.py: restores three tiny synthetic scenes with whichever build of the library
``SUCRE_HIP_LIB`` selects and prints, per scene,

  STORE <n> <format word of the compact store>
  RUNS <n> <kernel> <phase>,<rest> ...      the (ring slot of the first chunk, chunks mod 3) of every straight run (csrc/fit.hip,
                                            stream_strips' straight_run) the kernel takes in this scene: one, L, F
  NU <n> <strips> <strips without an unmasked full chunk>
  FIT <key> <md5 of the state block> <of the 27 parameter words> <of J> <of the trace>

so that two builds can be compared bit for bit and the test can see which entries of the unrolled loop the scenes reach.  The strips
are read back from the workspace's own plan (tests/native/plan_where.cpp, compiled by the test, says where it lies; argv[1])."""
import hashlib
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]

W, H = 64, 48
NEIGHBOURS = (9, 21, 44)
ITERATIONS = (5, 6)      # the odd one ends with the one-launch kernel
# what a strip's stream holds around its chunks, per kernel: (items before the chunks, chunks that take the per-chunk step because
# the wait still counts the last strip's stores, items behind the chunks)  -- stream_strips' kStart, kPeel, the moments
KERNELS = {'one': (1, 1, 1), 'L': (1, 1, 0), 'F': (3, 0, 0)}
RING = 3


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def wave_strips(r, where):
    """[[(unmasked full chunks, masked full chunks, levels of the short last chunk) of every strip of the wave, in its order]]."""
    out = subprocess.run([where, str(r.H), str(r.W), str(r.n_views)], capture_output=True, text=True, check=True).stdout.split()
    off_strips, off_count, kmax, waves, bits = (int(x) for x in out)
    torch.cuda.synchronize()
    count = r.ws[off_count:off_count + 4 * waves].cpu().numpy().view(np.uint32)
    entries = r.ws[off_strips:off_strips + 8 * waves * kmax].cpu().numpy().view(np.uint32).reshape(waves, kmax, 2)
    mask = (1 << bits) - 1
    return [[(int(c) & mask, (int(c) >> bits) & mask, (int(c) >> (2 * bits)) & 7) for c in entries[w, :count[w], 1]] for w in range(waves)]


def straight_runs(strips, kernel):
    """{(ring slot of the run's first chunk, its chunks mod 3)} over the waves' streams: the walk of stream_strips."""
    start, peel, end = KERNELS[kernel]
    runs = set()
    for wave in strips:
        i = 0
        for nu, nm, tail in wave:
            i += start + min(peel, nu)
            n = nu - min(peel, nu)
            if n:
                runs.add((i % RING, n % RING))
            i += n + nm + (1 if tail else 0) + end
    return runs


def restoration(n):
    from sucre_amd import engine, synth
    scene = synth.make_scene(W, H, n, seed=3 + n, device='cuda')
    views = engine.device_views_from_scene(scene, 'cuda')
    r = engine.Restoration(H, W, len(views))
    r.match(views[scene.target], views)
    return r, views[scene.target]


def report(key, r, trace):
    from sucre_amd import _lib
    torch.cuda.synchronize()
    s_off = r.lib.sucre_ws_offset(r.H, r.W, r.n_views, _lib.WS_STATE)
    n_strips = 4 * ((r.H + 15) // 16) * ((r.W + 15) // 16)
    state = r.ws[s_off:s_off + n_strips * 2304].cpu().numpy()            # J and both moments of every strip
    params = r._region(_lib.WS_PARAMS, torch.float32, 27).cpu().numpy()   # the nine parameters and their moments
    print('FIT', key, md5(state), md5(params), md5(r.J().cpu().numpy()), md5(trace.cpu().numpy()), flush=True)


def main():
    from sucre_amd import _lib
    where = sys.argv[1]
    print('LIB', _lib.LIB_PATH, flush=True)
    kept = {}
    for n in NEIGHBOURS:
        r, target = restoration(n)
        kept[n] = (r, target)
        print('STORE', n, int(r.store_format().cpu()[0]), flush=True)
        strips = wave_strips(r, where)
        for kernel in KERNELS:
            print('RUNS', n, kernel, *(f'{p},{m}' for p, m in sorted(straight_runs(strips, kernel))), flush=True)
        print('NU', n, sum(len(w) for w in strips), sum(nu == 0 for w in strips for nu, _, _ in w), flush=True)
        for T in ITERATIONS:
            for paired in (True, False):
                r.fit_init(target)
                report(f'{n}/T{T}/{"paired" if paired else "unpaired"}', r, r.fit(T, paired=paired))
    # two restorations in flight, each on its own stream
    pair = [kept[NEIGHBOURS[1]], kept[NEIGHBOURS[2]]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    traces = []
    for (r, target), st in zip(pair, streams):
        with torch.cuda.stream(st):
            r.fit_init(target)
            traces.append(r.fit(ITERATIONS[1]))
    torch.cuda.synchronize()
    for k, ((r, _), trace) in enumerate(zip(pair, traces)):
        report(f'inflight{k}', r, trace)


if __name__ == '__main__':
    main()
