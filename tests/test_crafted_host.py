"""The hand-built count histograms of tests/crafted.py on the CPU oracle: the inputs are ones the reference's arithmetic
passes, every bar ``Case.D`` is the oracle's own measured distance from the float64 model (held within [D/4, D]: it can neither
drift nor be inflated), and the checks are sharp -- each of four one-observation mutations of a store makes one of them fail.
tests/test_gpu_crafted.py holds the HIP engine to the same checks."""
import numpy as np
import pytest

import crafted
from crafted import CASE, CASES

IDS = [c.id for c in CASES]


def test_cases_have_the_histograms_they_were_chosen_for():
    def sorted_strips(c):
        s = np.sort(CASE[c].geometry().count_map().reshape(-1))[::-1]
        return s.reshape(-1, 64)
    for c, r in (('eq1', 1), ('eq2', 2), ('eq3', 3), ('eq4', 0), ('eq5', 1), ('eq8', 0)):
        cm = CASE[c].geometry().count_map()
        assert cm.min() == cm.max() and cm.max() % 4 == r
    g = CASE['stair'].geometry()
    cm = g.count_map().reshape(-1)
    assert all(len(set(cm[w * 64:(w + 1) * 64])) == 64 for w in range(4)) and cm.max() == 300 == g.n_views and g.n_obs == 32940
    s = sorted_strips('heavy')
    assert (s[0].max(), s[0].min()) == (64, 1)
    s = sorted_strips('straddle')
    assert s[0].tolist() == [6] + [5] * 63 and s[1].tolist() == [5] * 64 and s[2].tolist() == [5] + [4] * 63
    s = sorted_strips('straddle_mirror')
    assert s[1].tolist() == [5] * 64 and s[2].tolist() == [4] * 64 and s[3].tolist() == [4] * 63 + [3]
    g = CASE['edges'].geometry()
    assert sorted(set(g.view.tolist())) == [0, 63, 64, 127, 128, 191, 192, 199] and set(g.count_map().reshape(-1)) == set(range(1, 9))
    for n in (254, 255, 256):
        cm = CASE[f'bins{n}'].geometry().count_map()
        assert cm.max() == n and cm.min() <= 1
    g = CASE['maxviews'].geometry()
    assert g.n_views == 4096 and np.bincount(g.count_map().reshape(-1))[[0, 1, 15, 16, 17, 255, 4095, 4096]].tolist() == [32] * 8
    g = CASE['dropped'].geometry()
    assert g.kept.tolist() == [k not in (1, 4, 7, 10) for k in range(12)] and g.counts[[1, 4, 7, 10]].tolist() == [20] * 4
    assert g.n_obs == g.counts.sum() - 80
    for c in CASES:   # narrow ranges span fewer than 2^24 float32 bit patterns, wide ones more (and fewer than 2^26)
        for narrow in (False, True):
            b = c.geometry(narrow).z.view(np.uint32).astype(np.int64)
            assert (b.max() - b.min() <= 0xfffffd) == narrow and b.max() - b.min() <= 0x3fffffd


@pytest.mark.parametrize('cid', IDS)
def test_oracle_holds_the_identities_and_D_is_its_distance(cid):
    """Checks (a) and (c) on the oracle, on wide, narrow and millimetre ranges; the distances against the case's D."""
    case = CASE[cid]
    m = crafted.measure(case, crafted.oracle_backend)
    print(cid, ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
    assert (case.D['cJ'] is not None) == case.closed
    for k, x in m.items():
        assert case.D[k] / 4 <= x <= case.D[k], (cid, k, x, case.D[k])


@pytest.mark.parametrize('cid', IDS)
def test_oracle_exact_cost(cid):
    crafted.check_cost(CASE[cid].geometry(), crafted.oracle_backend(), cid)


def test_float_colour_round_on_the_oracle():
    for case in CASES:
        crafted.check_closed_form_float(case.geometry(), crafted.oracle_backend(), case.D['R'], case.id)


@pytest.mark.parametrize('kind', crafted.MUTATIONS)
@pytest.mark.parametrize('cid', ['stair', 'heavy', 'eq3'])
def test_one_mutated_observation_is_caught(cid, kind):
    case = CASE[cid]
    g = case.geometry()
    be = crafted.mutated(crafted.oracle_backend(), g, kind)
    caught = []
    for name, check in (('b', lambda: crafted.check_cost(g, be, cid)), ('a', lambda: crafted.check_closed_form(g, be, case.D['R'], cid))):
        try:
            check()
        except AssertionError as e:
            caught.append((name, str(e)[:200]))
    print(cid, kind, caught)
    assert caught, f'{kind} on {cid} passes checks (a) and (b)'
    # what each mutation is expected to trip: a lost observation the count, everything else an identity of check (a)
    assert ('b' if kind == 'drop' else 'a') in [n for n, _ in caught]
