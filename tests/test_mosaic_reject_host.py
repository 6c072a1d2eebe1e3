"""Host tests (no GPU) of the mosaic's colour consensus across views: the value check, the refusals and the accepted combinations,
the keyword's place, the count picture, the crafted survey's claims on the restatement (tests/mosaic_reject_ref.py), the restatement
against plain loops over the definition, and the claim's chain of atomic minima of csrc/reject.h under random interleavings."""
import inspect
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_reject_crafted as crafted
import mosaic_reject_ref as rref
import mosaic_support_ref as pref
from sucre_amd import _lib, engine, sucre
from test_mosaic_gains_host import answer, small_survey

FREE = 0xffffffff


# ---- the value, the refusals and the keyword's place -----------------------------------------------------------------------------------

def test_the_tolerance_is_checked_like_the_other_values():
    assert engine.MOSAIC_REJECT_RANGE == (1e-6, 1e6)
    assert _lib.MOSAIC_REJECT_CELL_IMAGES == 8 == rref.SLOTS and _lib.MOSAIC_REJECT_MIN_VIEWS == 3 == rref.MIN_VIEWS
    def checked(reject, who):
        return engine.MosaicOptions(reject=reject).checked(who).reject
    assert checked(None, 'x') is None
    for good in (1e-6, 0.15, 1, 1e6, np.float32(1e-6), '0.5'):
        T = checked(good, 'x')
        assert engine.mosaic_reject_tol(good) == T and type(engine.mosaic_reject_tol(good)) is np.float32
        assert type(T) is np.float32 and T == np.float32(float(good))
    for bad in (0, -0.1, 5e-7, 1.0000001e6, float('nan'), float('inf'), 'T', ()):
        with pytest.raises(ValueError, match=r'mosaic reject tolerance T must be finite and within \[1e-06, 1e\+06\] colour units') as e:
            checked(bad, 'x')
        assert e.value.field == 'reject'
    view = SimpleNamespace(depth=SimpleNamespace(device=torch.device('cpu')))
    with pytest.raises(ValueError, match='reject tolerance') as e:       # before a Mosaic is made
        engine.mosaic_of([view], [None], torch.eye(3), 0.1, reject=0)
    assert e.value.field == 'reject'


def test_the_keyword_stands_ahead_of_the_last_one_and_the_tables_keep_their_rows():
    names = list(inspect.signature(sucre.mosaic).parameters)
    assert names[-2:] == ['reject', 'gain_solve'] and inspect.signature(sucre.mosaic).parameters['reject'].default is None
    for f in (engine.mosaic_of, engine.Mosaic.run, engine.Mosaic.begin):      # these take it as a field of the record
        assert list(inspect.signature(f).parameters.values())[-1].kind is inspect.Parameter.VAR_KEYWORD, f
    assert engine.MosaicOptions().reject is None and engine.MosaicOptions().over(reject=0.5).reject == 0.5
    for name in ('sucre_mosaic_reject_claim', 'sucre_mosaic_reject_sums', 'sucre_mosaic_reject_consensus', 'sucre_mosaic_reject_cull'):
        assert name in _lib.SIGNATURES
    for name in ('add_reject_claim', 'add_reject_sums', 'finish_reject', 'rejected_images'):
        assert callable(getattr(engine.Mosaic, name))
    assert list(engine.MOSAIC_OUTPUTS)[-9:-5] == ['support', 'surface_source', 'culled_above', 'surface_top']
    assert list(engine.MOSAIC_OUTPUTS)[-5:] == list(engine.MOSAIC_REJECT_OUTPUTS)      # the rows of the one table, its last group
    assert [k for k, row in engine.MOSAIC_OUTPUTS.items() if row[0] == 'reject'] == list(engine.MOSAIC_REJECT_OUTPUTS)
    assert list(engine.MOSAIC_REJECT_OUTPUTS) == ['rejected', 'reject_ref', 'reject_source', 'reject_views', 'reject_overflow']
    assert all(len(row) == 6 and row[0] == 'reject' for row in engine.MOSAIC_REJECT_OUTPUTS.values())
    assert engine.MOSAIC_REJECT_OUTPUTS['rejected'][4:] == ('mosaic_rejected.png', 'count')
    assert all(engine.MOSAIC_OUTPUTS[k] is row for k, row in engine.MOSAIC_REJECT_OUTPUTS.items())
    assert [f.name for f in engine.MosaicOptions.__dataclass_fields__.values()] == ['blend', 'feather', 'fill', 'bands', 'surface', 'support', 'gains', 'gain_limit', 'gain_solve', 'reject']
    assert list(engine.MOSAIC_VALUES) == ['blend', 'fill', 'feather', 'bands', 'surface', 'support', 'gains', 'gain_limit', 'gain_solve', 'reject']
    assert engine.MOSAIC_VALUES['reject'] == ('reject tolerance T', (1e-6, 1e6), False, 'colour units', np.float32, 'T', 'a finite tolerance')
    assert engine.MOSAIC_VALUES['reject'][1] is engine.MOSAIC_REJECT_RANGE
    assert len(sucre._ONLY_WITH) == 11 and sucre._ONLY_WITH[-1] == ('--mosaic-reject', '--mosaic', 'DIR')
    assert sucre._MOSAIC_FLAG['reject'] == '--mosaic-reject'


def test_the_command_line_refuses_before_any_file_is_opened(monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert answer(['--mosaic-reject', '0.15']) == '--mosaic-reject: only with --mosaic DIR'
    # the table's rows are looked at first
    assert answer(['--mosaic-reject', '0.15', '--mosaic-surface', '0.1']) == '--mosaic-surface: only with --mosaic DIR'
    assert answer(['--mosaic-reject', '0.15', '--mosaic-gain-solve', 'direct']) == '--mosaic-gain-solve: only with --mosaic-gains R'
    for bad, shown in (('0', '0.0'), ('nan', 'nan'), ('2e6', '2000000.0'), ('-1', '-1.0'), ('inf', 'inf')):
        assert answer(['--mosaic', 'results', '--mosaic-reject', bad]) == \
            f'--mosaic-reject: T must be a finite tolerance within [1e-06, 1e+06] colour units, not {shown}'
    for good in ([], ['--mosaic-blend', '0.5', '--mosaic-feather', '8', '--mosaic-bands', '2', '--mosaic-fill', '0.1'],
                 ['--mosaic-surface', '0.1', '--mosaic-support', '2'], ['--mosaic-gains', '2', '--mosaic-gain-solve', 'direct'],
                 ['--mosaic-gsd', '0.05']):
        assert answer(['--mosaic', 'results', '--mosaic-reject', '0.15'] + good) == 'accepted', good
    assert answer(['--mosaic', 'results', '--mosaic-reject', '1e-6']) == 'accepted'
    assert answer(['--mosaic', 'results', '--mosaic-reject', '1e6']) == 'accepted'


def test_the_python_entry_refuses_like_the_command_line(monkeypatch):
    monkeypatch.setattr(sucre.sfm, 'require_gpu', lambda device, what: None)
    image = SimpleNamespace(name='a.png')
    with pytest.raises(SystemExit) as e:
        sucre.mosaic([image], None, 'results', 'out', reject=0)
    assert e.value.code == '--mosaic-reject: mosaic reject tolerance T must be finite and within [1e-06, 1e+06] colour units, not 0'


def test_the_count_picture_is_the_culled_one():
    counts = np.array([[0, 1, 2], [4, 0, 3]], np.int32)
    assert np.array_equal(sucre.mosaic_culled_picture(counts), np.array([[0, 63, 127], [255, 0, 191]], np.uint8))
    assert not sucre.mosaic_culled_picture(np.zeros((2, 2), np.int32)).any()
    assert sucre._MOSAIC_PNG[engine.MOSAIC_REJECT_OUTPUTS['rejected'][5]] is sucre._MOSAIC_PNG['count']


# ---- the crafted survey on the restatement ---------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def fish():
    views, Js = crafted.survey()
    return views, Js, rref.reject(views, Js, torch.eye(3), crafted.GSD, crafted.TOL)


def test_the_height_tests_cannot_see_the_fish(fish):
    views, Js, _ = fish
    out = pref.support(views, Js, torch.eye(3), crafted.GSD, 0.1, 2)
    assert out['counts'][:2] == (0, 0) and not bool(out['culled'].any()) and not bool(out['culled_above'].any())


def test_exactly_the_fish_is_rejected(fish):
    views, Js, out = fish
    mask = crafted.fish_mask()
    assert int(mask.sum()) == crafted.N_FISH == 384
    assert np.array_equal(out['mask'][crafted.FISH_VIEW], mask) and not out['mask'][0].any() and not out['mask'][2].any()
    assert out['per_image'][:, 1].tolist() == [0, crafted.N_FISH, 0] and int(out['rejected'].sum()) == crafted.N_FISH
    assert not bool(out['reject_overflow'].any()) and int(out['reject_views'].max()) == 3
    p, cells = out['cells'][crafted.FISH_VIEW]
    fish_cells = np.unique(cells[mask.reshape(-1)[p]])
    source = out['reject_source'].numpy().reshape(-1)
    assert set(source[fish_cells].tolist()) <= {0, 2}                                    # never the fish's view
    # the plane means tie and order by ordinal: of three plane images the lower median is ordinal 1; where view 1 holds a fish
    # sample it is the brightest and the median is ordinal 2
    three = out['reject_views'].numpy().reshape(-1) == 3
    assert bool(three[fish_cells].all())
    assert set(source[three].tolist()) == {1, 2} and set(source[fish_cells].tolist()) == {2}
    assert bool((source[~three] == -1).all()) and int((~three).sum()) > 0             # the rim: one or two views, no consensus
    # the reference is the plane colour to within half a quantiser step
    ref = out['reject_ref'].numpy().reshape(-1, 3)
    assert float(np.abs(ref[three] - np.float32(0.4)).max()) <= 2.0 ** -15 and bool(np.isnan(ref[~three]).all())
    # the copies: NaN exactly at the fish
    for i, (J, Jc) in enumerate(zip(Js, out['Js'])):
        gone = np.isnan(Jc.numpy()).all(axis=2)
        assert np.array_equal(gone, mask if i == crafted.FISH_VIEW else np.zeros_like(mask))
        assert np.array_equal(Jc.numpy()[~gone], J.numpy()[~gone])


def test_two_views_reject_nothing_whatever_they_hold():
    views, Js = crafted.survey()
    out = rref.reject(views[:2], Js[:2], torch.eye(3), crafted.GSD, 1e-6)
    assert int(out['reject_views'].max()) == 2 and bool((out['reject_source'] == -1).all()) and not bool(out['rejected'].any())
    assert out['per_image'].tolist() == [[0, 0], [0, 0]]


# ---- the restatement against plain loops -----------------------------------------------------------------------------------------------

def test_the_restatement_equals_plain_loops_over_the_definition():
    views, Js = small_survey()
    views, Js = views + views[:3] * 2 + [views[0]], Js + Js[:3] * 2 + [Js[0]]            # 12 ordinals: cells overflow
    axes, gsd, T = torch.eye(3), 0.2, 0.3
    out = rref.reject(views, Js, axes, gsd, T)
    n_cells = out['Hm'] * out['Wm']
    reach = [dict() for _ in range(n_cells)]                                              # cell -> ordinal -> [n, S0, S1, S2]
    for i, ((p, cells), J) in enumerate(zip(out['cells'], Js)):
        x = J.numpy().reshape(-1, 3)
        for px, c in zip(p.tolist(), cells.tolist()):
            row = reach[c].setdefault(i, [0, 0, 0, 0])
            row[0] += 1
            for ch in range(3):
                v = np.float32(x[px, ch])
                q = np.float32(min(max(v, np.float32(-8)), np.float32(8))) * np.float32(16384)
                row[1 + ch] += int(np.rint(q))
    assert int(out['slot_over'].sum()) > 0 and int((out['slot_over'] == 0).sum()) > 0
    n_ref = 0
    for c in range(n_cells):
        ords = sorted(reach[c])
        kept = ords[:8]
        assert out['slot_ord'][c].tolist() == kept + [FREE] * (8 - len(kept))
        assert int(out['slot_over'][c]) == (1 if len(ords) > 8 else 0)
        for a, o in enumerate(kept):
            assert out['slot_sum'][c, a].tolist() == reach[c][o]
        assert not out['slot_sum'][c, len(kept):].any()
        assert int(out['reject_views'].reshape(-1)[c]) == len(kept)
        if len(kept) < 3:
            assert int(out['reject_source'].reshape(-1)[c]) == -1
            continue
        # the order by cross-multiplied integers, as the kernel compares
        def before(a, b):
            Ya, Yb = sum(reach[c][a][1:]), sum(reach[c][b][1:])
            l, r = Ya * reach[c][b][0], Yb * reach[c][a][0]
            return l < r or (l == r and a < b)
        order = sorted(kept, key=lambda a: sum(before(b, a) for b in kept if b != a))
        src = order[(len(kept) - 1) // 2]
        assert int(out['reject_source'].reshape(-1)[c]) == src
        n_ref += 1
    assert n_ref > 0
    gone = sum(int(m.sum()) for m in out['mask'])
    assert 0 < gone == int(out['rejected'].sum()) == int(out['per_image'][:, 1].sum()) < int(out['per_image'][:, 0].sum())
    # a sample of the reference image is never rejected, and an image outside an overflowed cell's eight is tested all the same
    source = out['reject_source'].numpy().reshape(-1)
    late = 0
    for i, ((p, cells), mask) in enumerate(zip(out['cells'], out['mask'])):
        hit = mask.reshape(-1)[p]
        assert not bool(hit[source[cells] == i].any())
        late += int(hit.sum()) if i >= 8 else 0
    assert late > 0


# ---- the claim's chain under random interleavings ----------------------------------------------------------------------------------------

def run_lanes(values, rng, filtered):
    """Every value's lane steps through the chain, one atomic step at a time, in a random interleaving; ``filtered``: a lane first
    reads the eight words, each at a moment of its own (a step of the schedule per word), and acts as the default form does."""
    words, flag = [FREE] * 8, [0]

    def lane(v):
        start = 0
        if filtered:
            seen = []
            for s in range(8):
                seen.append(words[s])
                yield
            if v in seen:
                return
            bigger = [s for s in range(8) if seen[s] > v]
            if not bigger:
                flag[0] = 1
                return
            start = bigger[0]
        if (yield from rref.chain_steps(words, v, start)):
            flag[0] = 1

    live = [lane(v) for v in values]
    while live:
        g = rng.choice(live)
        try:
            next(g)
        except StopIteration:
            live.remove(g)
        for s in range(7):      # at EVERY moment: strictly ascending unless the next word is free
            assert words[s] < words[s + 1] or words[s + 1] == FREE, words
    return words, flag[0]


@pytest.mark.parametrize('filtered', [False, True])
def test_the_chain_ends_in_the_sorted_prefix_under_any_interleaving(filtered):
    rng = random.Random(17 + filtered)
    seen_flag = set()
    for trial in range(300):
        n = rng.randint(1, 12)
        distinct = rng.sample(range(40), n)
        values = distinct + [rng.choice(distinct) for _ in range(rng.randint(0, 6))]       # several lanes carry one ordinal
        rng.shuffle(values)
        words, flag = run_lanes(values, rng, filtered)
        want = sorted(distinct)[:8]
        assert words == want + [FREE] * (8 - len(want)), (trial, values, words)
        assert flag == (1 if n > 8 else 0), (trial, values)
        seen_flag.add(flag)
    assert seen_flag == {0, 1}
