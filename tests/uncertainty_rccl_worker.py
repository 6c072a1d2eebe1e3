"""``sucre.pooled_uncertainty`` over RCCL on the one-GPU box (tests/test_gpu_uncertainty_rccl.py): a process group of ONE rank over
backend 'nccl' with ``dist.COLLECTIVE_AT_WORLD_1`` set, so that the all-reduce of the 24 words really goes through RCCL -- which
takes device tensors only: a host tensor handed to it raises.  A sum over one rank is the identity, so the pooled words must
equal the plain sum bit for bit, for sums that live on the device (what ``restore_shared_water`` passes) and for host sums."""
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]


def main() -> None:
    import torch.distributed as dist
    from sucre_amd import dist as sdist
    from sucre_amd import engine, sucre, synth
    scene = synth.make_scene(64, 48, 4, seed=21, device='cuda')
    views = engine.device_views_from_scene(scene, 'cuda')
    parts = []
    for target in (scene.target, (scene.target + 1) % len(views), (scene.target + 2) % len(views)):
        r = engine.Restoration(scene.height, scene.width, len(views), device='cuda')
        r.match(views[target], views)
        r.fit_init(views[target])
        r.fit(10)
        parts.append(r.uncertainty()[2])
    assert all(p.is_cuda for p in parts)
    plain = (parts[0].cpu() + parts[1].cpu()) + parts[2].cpu()
    assert not dist.is_initialized() and torch.equal(sucre.pooled_uncertainty(parts), plain)
    os.environ.update(RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29533')
    sdist.COLLECTIVE_AT_WORLD_1 = True
    sdist.init_process_group(backend='nccl')
    assert dist.is_initialized() and dist.get_backend() == 'nccl' and dist.get_world_size() == 1
    calls = []
    real = dist.all_reduce

    def counting(t, *a, **k):
        calls.append((t.dtype, t.is_cuda, int(t.numel())))
        return real(t, *a, **k)
    dist.all_reduce = counting
    try:
        for label, given in (('device sums', parts), ('host sums', [p.cpu() for p in parts])):
            calls.clear()
            total = sucre.pooled_uncertainty(given)
            assert calls == [(torch.float64, True, 24)], (label, calls)          # one reduce, of the 24 words, on the device
            assert not total.is_cuda and total.dtype == torch.float64 and torch.equal(total, plain), (label, total, plain)
    finally:
        dist.all_reduce = real
    res = engine.water_uncertainty(total)
    assert res['n_obs'] == int(plain[0]) and res['well_posed'].all()
    print(f'RCCL_POOL_OK backend={dist.get_backend()} world={dist.get_world_size()} N={res["n_obs"]} P={res["n_pixels"]}', flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
