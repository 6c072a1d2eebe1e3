"""Child process of tests/test_gpu_staged.py: fits the hand-built stores of tests/crafted.py with whichever build of the library
``SUCRE_HIP_LIB`` selects and prints one line per fit -- ``FIT <key> <md5 of the state block> <of the 27 parameter words> <of J>
<of the trace>`` -- so that two builds can be compared bit for bit.  Six iterations each, from the same seeded J0 (NaN where
nobody observes the pixel); the J-parameter mode through every launch that runs the chunk arithmetic of csrc/fit.hip (accumulate_chunk;
experiment.h SUCRE_STAGED_TERMS): ``fit`` in pairs (L and F) and one launch per iteration, a group of one (group_iter_kernel), and
a ``fit_batch`` of two images (batch_iter_kernel, whose text the knob leaves alone)."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]

T = 6
# tail only (eq1), three levels, exactly one full chunk (eq4), a full chunk + a tail (eq5), 64 distinct counts in a wave and a
# masked chunk in every strip (stair), levels = 64 next to full = 1 (heavy), strips of 0 .. 8 levels with slots outside the image
# (ragged: masked chunks), and a strip nobody observes (unseen: NaN J)
CASES = ('eq1', 'eq3', 'eq4', 'eq5', 'stair', 'heavy', 'ragged40x24', 'ragged80x16', 'unseen')
FORMATS = ('f32', 'u16mm')
P_IN = np.full(9, 0.1, np.float32)                                            # B inside scaled_b_ok's window: the B-scaled form
P_ZERO = np.array([0.1, 0.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1], np.float32)  # one channel of B is 0: the whole launch runs the fallback
PARAMS = (('scaled', P_IN), ('fallback', P_ZERO))


def geometry(cid, fmt):
    """'f32' runs on the narrow ranges, where the default store picks 24-bit codes; 'u16mm' on the wide ones."""
    import crafted
    narrow = fmt == 'f32'
    if cid != 'unseen':
        return crafted.CASE[cid].geometry(narrow=narrow)
    key = ('staged_unseen', narrow)   # 16x16: strips of 5, 4 (masked: 32 pixels have three), 1 and 0 levels
    if key not in crafted._GEOMS:
        cnt = np.concatenate([np.full(64, 5), np.full(32, 4), np.full(32, 3), np.full(64, 1), np.full(64, 0)])
        crafted._GEOMS[key] = crafted.build(16, 16, 8, cnt[np.random.default_rng(3).permutation(256)], seed=2, narrow=narrow)
    return crafted._GEOMS[key]


def partner(g, fmt):
    """Another store of the same size for a launch over two images: 'heavy' next to a 16x16 store, the stair run backwards (other
    views, other ranges) next to a ragged one."""
    import crafted
    narrow = fmt == 'f32'
    if (g.H, g.W) == (16, 16):
        return crafted.CASE['heavy'].geometry(narrow=narrow)
    key = ('staged_partner', g.H, g.W, narrow)
    if key not in crafted._GEOMS:
        crafted._GEOMS[key] = crafted.build(g.H, g.W, 8, 8 - crafted._stair9(g.H * g.W, None), seed=6, narrow=narrow)
    return crafted._GEOMS[key]


def load(g, fmt, p0):
    import crafted
    from sucre_amd import engine
    r = engine.Restoration(g.H, g.W, g.n_views, obs_format=fmt)
    J0 = (3.0 + np.random.default_rng(11).random((g.H, g.W, 3))).astype(np.float32)
    J0[g.count_map() == 0] = np.nan
    crafted.EngineBackend(r)._load(r, crafted.ListSet(g, rgb=crafted.random_colours(g)), p0, J0)
    return r


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def report(key, r, trace):
    from sucre_amd import _lib
    torch.cuda.synchronize()
    s_off = r.lib.sucre_ws_offset(r.H, r.W, r.n_views, _lib.WS_STATE)
    n_strips = 4 * ((r.H + 15) // 16) * ((r.W + 15) // 16)
    state = r.ws[s_off:s_off + n_strips * 2304].cpu().numpy()            # J and both moments of every strip
    params = r._region(_lib.WS_PARAMS, torch.float32, 27).cpu().numpy()   # the nine parameters and their moments
    print('FIT', key, md5(state), md5(params), md5(r.J().cpu().numpy()), md5(trace.cpu().numpy()), flush=True)


def main():
    from sucre_amd import _lib, engine
    from sucre_amd import dist as sdist
    print('LIB', _lib.LIB_PATH, flush=True)
    for cid in CASES:
        for fmt in FORMATS:
            g = geometry(cid, fmt)
            for pname, p0 in PARAMS:
                for paired in (True, False):
                    r = load(g, fmt, p0)
                    report(f'{cid}/{fmt}/{pname}/{"paired" if paired else "unpaired"}', r, r.fit(T, paired=paired))
                r = load(g, fmt, p0)
                trace = torch.zeros((T, 10), dtype=torch.float64, device='cuda')
                sdist.fit_shared_water(engine.HipWaterGroup([r], lr=0.05, use_closed_form=False, trace=trace, params0=p0), T)
                report(f'{cid}/{fmt}/{pname}/group', r, trace)
                # a batch launch over two images
                r, r2 = load(g, fmt, p0), load(partner(g, fmt), fmt, p0)
                traces = engine.fit_batch([r, r2], T)
                report(f'{cid}/{fmt}/{pname}/batch0', r, traces[0])
                report(f'{cid}/{fmt}/{pname}/batch1', r2, traces[1])


if __name__ == '__main__':
    main()
