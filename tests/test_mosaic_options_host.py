"""Host tests of ``engine.MosaicOptions``: ``checked()`` against the ten public validators on the ends of every range, the one
order of its refusals, and the numbers of the command line's refusals against ``engine.MOSAIC_VALUES``.  No GPU."""
import argparse
import dataclasses

import numpy as np
import pytest

from sucre_amd import engine, sucre

NAN, INF = float('nan'), float('inf')
FIELDS = ['blend', 'feather', 'fill', 'bands', 'surface', 'support', 'gains', 'gain_limit', 'gain_solve', 'reject']      # the record's order
TABLE = ['blend', 'fill', 'feather', 'bands', 'surface', 'support', 'gains', 'gain_limit', 'gain_solve', 'reject']       # the order checked
NUMBERS = [f for f in TABLE if f != 'gain_solve']
VALIDATOR = {'blend': engine.mosaic_blend_depth, 'fill': engine.mosaic_fill_reach, 'feather': engine.mosaic_feather_px,
             'bands': engine.mosaic_band_count, 'surface': engine.mosaic_surface_tol, 'support': engine.mosaic_support_views,
             'gains': engine.mosaic_gain_rounds, 'gain_limit': engine.mosaic_gain_limit, 'gain_solve': engine.mosaic_gain_solve_name,
             'reject': engine.mosaic_reject_tol}
KIND = {'blend': np.float32, 'fill': float, 'feather': int, 'bands': int, 'surface': np.float32, 'support': int, 'gains': int,
        'gain_limit': float, 'gain_solve': str, 'reject': np.float32}
RANGE = {'blend': engine.MOSAIC_BLEND_RANGE, 'fill': engine.MOSAIC_FILL_RANGE, 'feather': engine.MOSAIC_FEATHER_RANGE,
         'bands': engine.MOSAIC_BANDS_RANGE, 'surface': engine.MOSAIC_SURFACE_RANGE, 'support': engine.MOSAIC_SUPPORT_RANGE,
         'gains': engine.MOSAIC_GAIN_ROUNDS_RANGE, 'gain_limit': engine.MOSAIC_GAIN_LIMIT_RANGE, 'gain_solve': engine.MOSAIC_GAIN_SOLVES,
         'reject': engine.MOSAIC_REJECT_RANGE}
GOOD = {'blend': [1e-6, 1e6, 0.5, '0.5', np.float32(2)], 'fill': [1e-6, 1e6, 0.05, '3', np.float64(2)], 'feather': [1, 1024, 8.0, '16', np.int64(3)],
        'bands': [1, 6, 4.0, '3', np.int64(2)], 'surface': [1e-6, 1e6, 0.05, '0.5', np.float32(2)], 'support': [1, 4, 3.0, '2', np.int64(2)],
        'gains': [1, 64, 3.0, '16', np.int64(2)], 'gain_limit': [1, 16, 2.5, '4', np.float32(4)], 'gain_solve': ['direct'],
        'reject': [1e-6, 1e6, 0.15, '0.5', np.float32(2)]}
REAL_BAD = [9.9e-7, 1.0000001e6, 0.0, -1.0, NAN, INF, -INF]
BAD = {'blend': REAL_BAD + ['deep'], 'fill': REAL_BAD + ['far'], 'feather': [0, 1025, -3, NAN, INF, True, False, 2.5, 1.5, 'wide'],
       'bands': [0, 7, -1, NAN, INF, True, False, 2.5, 1e9, 'many'], 'surface': REAL_BAD + ['x'],
       'support': [0, 5, -1, NAN, INF, True, False, 2.5, 'x'], 'gains': [0, 65, -1, NAN, INF, True, False, 2.5, 'x'],
       'gain_limit': [0.99, 16.5, 0, -2, NAN, INF, -INF, 'x'], 'gain_solve': ['Direct', 'exact', '', 1, True, 2.5],
       'reject': REAL_BAD + ['T', ()]}
TEXT = {'blend': 'mosaic blend depth H must be finite and within [1e-06, 1e+06] metres, not {}',
        'fill': 'mosaic fill reach R must be finite and within [1e-06, 1e+06] metres, not {}',
        'feather': 'mosaic feather width F must be an integer within [1, 1024] source pixels, not {}',
        'bands': 'mosaic band count K must be an integer within [1, 6] bands, not {}',
        'surface': 'mosaic surface tolerance T must be finite and within [1e-06, 1e+06] metres, not {}',
        'support': 'mosaic supporting views M must be an integer within [1, 4] views, not {}',
        'gains': 'mosaic gain rounds R must be an integer within [1, 64] rounds, not {}',
        'gain_limit': 'mosaic gain limit L must be finite and within [1, 16] times, not {}',
        'gain_solve': 'mosaic gain solve must be one of rounds or direct, not {!r}',
        'reject': 'mosaic reject tolerance T must be finite and within [1e-06, 1e+06] colour units, not {}'}
PARTNER = {'feather': {'blend': 0.5}, 'bands': {'blend': 0.5}, 'support': {'surface': 0.1}, 'gain_limit': {'gains': 3}, 'gain_solve': {'gains': 3}}
NEEDS = {'feather': 'a feather is a factor of the blend\'s weight; give the blend depth too (blend=H)',
         'bands': 'the bands are blended with the blend\'s weights; give the blend depth too (blend=H)',
         'support': 'the support decides which top the surface test measures against; give the tolerance too (surface=T)',
         'gain_limit': 'the limit clamps the gains the rounds find; give the rounds too (gains=R)',
         'gain_solve': 'the solve finds the gains of the first round; give the rounds too (gains=R)'}


def options(field, value):
    """The record with ``value`` in ``field`` -- and next to it the option it only goes with, where there is one."""
    return engine.MosaicOptions(**PARTNER.get(field, {}), **{field: value})


def cast(field, value):
    """What a checked ``value`` is: the number as the field's type, a choice itself."""
    return value if field == 'gain_solve' else KIND[field](float(value))


def test_the_table_holds_the_public_ranges():
    assert list(engine.MOSAIC_VALUES) == TABLE      # the order in which checked() looks at them
    assert [f.name for f in dataclasses.fields(engine.MosaicOptions)] == FIELDS
    assert all(f.default is None for f in dataclasses.fields(engine.MosaicOptions))
    for field in TABLE:
        assert engine.MOSAIC_VALUES[field][1] is RANGE[field] and engine.MOSAIC_VALUES[field][4] is KIND[field] and len(engine.MOSAIC_VALUES[field]) == 7
    assert engine.MOSAIC_BLEND_RANGE == engine.MOSAIC_FILL_RANGE == engine.MOSAIC_SURFACE_RANGE == engine.MOSAIC_REJECT_RANGE == (1e-6, 1e6)
    assert engine.MOSAIC_FEATHER_RANGE == (1, 1024) and engine.MOSAIC_BANDS_RANGE == (1, 6) and engine.MOSAIC_SUPPORT_RANGE == (1, 4)
    assert engine.MOSAIC_GAIN_ROUNDS_RANGE == (1, 64) and engine.MOSAIC_GAIN_LIMIT_RANGE == (1.0, 16.0) and engine.MOSAIC_GAIN_SOLVES == ('rounds', 'direct')
    assert [row[5] for row in engine.MOSAIC_VALUES.values()] == ['H', 'R', 'F', 'K', 'T', 'M', 'R', 'L', 'S', 'T']      # the command line's letters
    assert [row[2] for row in engine.MOSAIC_VALUES.values()] == [False, False, True, True, False, True, True, False, None, False]
    assert [row[:2] for row in engine.MOSAIC_NEEDS] == [('feather', 'blend'), ('bands', 'blend'), ('support', 'surface'), ('gain_limit', 'gains'),
                                                        ('gain_solve', 'gains')]
    assert {row[0]: row[2] for row in engine.MOSAIC_NEEDS} == NEEDS
    assert engine.MosaicOptions() == engine.MosaicOptions(None, None, None) == engine.MosaicOptions(*[None] * 10) == engine.MosaicOptions().checked()
    with pytest.raises(dataclasses.FrozenInstanceError):
        engine.MosaicOptions().blend = 1.0
    with pytest.raises(dataclasses.FrozenInstanceError):
        engine.MosaicOptions().reject = 1.0


def test_fields_are_laid_over_a_record_and_an_unknown_name_is_a_type_error():
    base = engine.MosaicOptions(blend=0.5, fill=0.1)
    assert base.over() is base and base.over(feather=8, fill=None) == engine.MosaicOptions(blend=0.5, feather=8)
    assert base.asked() == {'blend': 0.5, 'fill': 0.1} and engine.MosaicOptions().asked() == {}
    assert list(engine.MosaicOptions(*range(1, 11)).asked()) == FIELDS
    with pytest.raises(TypeError):
        base.over(blur=3)


@pytest.mark.parametrize('field', TABLE)
def test_checked_takes_what_the_validator_takes_and_returns_its_type(field):
    for value in GOOD[field]:
        want = VALIDATOR[field](value)
        got = getattr(options(field, value).checked(), field)
        assert type(want) is KIND[field] and type(got) is KIND[field] and got == want == cast(field, value), value
        assert options(field, value).checked().checked() == options(field, value).checked()      # at the ends of the range too
    both = engine.MosaicOptions(blend='0.25', feather=4.0, fill=np.float32(0.5)).checked()
    assert (both.blend, both.feather, both.fill) == (np.float32(0.25), 4, 0.5)
    assert [type(x) for x in (both.blend, both.feather, both.fill)] == [np.float32, int, float]
    assert both.checked() == both


def test_checked_returns_all_ten_as_their_types_and_fills_in_the_limit():
    full = engine.MosaicOptions(blend='0.25', feather=4.0, fill=np.float32(0.5), bands='2', surface=0.05, support=2.0, gains=3.0, gain_limit=4,
                                gain_solve='direct', reject='0.15').checked()
    assert dataclasses.astuple(full) == (np.float32(0.25), 4, 0.5, 2, np.float32(0.05), 2, 3, 4.0, 'direct', np.float32(0.15))
    assert [type(x) for x in dataclasses.astuple(full)] == [KIND[f] for f in FIELDS]
    assert full.checked() == full and full.checked('anyone') == full
    # the limit unless one is given, and only with gains; 'rounds' is the rounds alone
    assert engine.MosaicOptions(gains=3).checked() == engine.MosaicOptions(gains=3, gain_limit=engine.MOSAIC_GAIN_LIMIT) and engine.MOSAIC_GAIN_LIMIT == 2.0
    assert type(engine.MosaicOptions(gains=3).checked().gain_limit) is float and engine.MosaicOptions().checked().gain_limit is None
    rounds = engine.MosaicOptions(gains=3, gain_solve='rounds').checked()
    assert rounds.gain_solve is None and rounds == engine.MosaicOptions(gains=3).checked() == rounds.checked()
    assert engine.mosaic_gain_solve_name('rounds') == 'rounds'


@pytest.mark.parametrize('field', TABLE)
def test_checked_refuses_what_the_validator_refuses_with_its_text(field):
    for value in BAD[field] + [None]:
        with pytest.raises(ValueError) as want:
            VALIDATOR[field](value)
        assert str(want.value) == TEXT[field].format(value) and want.value.needs is None
        if value is None:      # in the record: not asked for
            continue
        with pytest.raises(ValueError) as got:
            options(field, value).checked()
        assert str(got.value) == str(want.value) and got.value.field == field == want.value.field and got.value.needs is None


@pytest.mark.parametrize('field', ['blend', 'fill', 'surface', 'reject'])
def test_the_ends_of_a_range_are_compared_in_float64(field):
    """Written out here, not taken from the engine: finite and ``lo <= float(value) <= hi`` in float64, as before the record."""
    lo, hi = 1e-6, 1e6
    near = [lo, hi, np.nextafter(lo, 0.0), np.nextafter(lo, 1.0), np.nextafter(hi, 0.0), np.nextafter(hi, np.inf), 9.99999998e-7, 1000000.01,
            1000000.03, float(np.float32(1e-6)), np.float64(np.float32(1e-6)), np.float64(1e-6), str(float(np.float32(1e-6))), '1e-6']
    for value in near:
        takes = lo <= float(value) <= hi
        for check in (VALIDATOR[field], lambda v: getattr(options(field, v).checked(), field)):
            if takes:
                assert check(value) == KIND[field](float(value)), value
            else:
                with pytest.raises(ValueError) as e:
                    check(value)
                assert str(e.value) == TEXT[field].format(value)
    assert [lo <= float(v) <= hi for v in near] == [True, True, False, True, True, False, False, False, False, False, False, True, False, True]


def test_a_float32_blend_depth_meets_the_ends_as_float32_rounds_them():
    """The one value this sets apart: float32(1e-6) lies below 1e-6, and it is what ``checked()`` makes of 1e-6 -- a checked record
    has to pass ``Mosaic.begin``, which checks again.  Only a value that IS a float32; the same number as a float stays refused, and
    so does a float32 reach, which is not the type of a checked reach.  The two float32 tolerances are as the blend depth."""
    low = np.float32(1e-6)
    assert float(low) < 1e-6 and engine.mosaic_blend_depth(low) == low and type(engine.mosaic_blend_depth(low)) is np.float32
    once = engine.MosaicOptions(blend=1e-6, surface=1e-6, reject=1e-6).checked()
    assert [type(x) for x in (once.blend, once.surface, once.reject)] == [np.float32] * 3 and once.checked() == once
    assert engine.mosaic_blend_depth(np.float32(1e6)) == np.float32(1e6)
    for bad in (float(low), np.float64(low), np.nextafter(low, np.float32(0)), np.nextafter(np.float32(1e6), np.float32(np.inf))):
        with pytest.raises(ValueError, match='blend depth H'):
            engine.mosaic_blend_depth(bad)
        with pytest.raises(ValueError, match='surface tolerance T'):
            engine.mosaic_surface_tol(bad)
        with pytest.raises(ValueError, match='reject tolerance T'):
            engine.mosaic_reject_tol(bad)
    with pytest.raises(ValueError, match='fill reach R'):
        engine.mosaic_fill_reach(low)


def test_checked_looks_at_blend_then_fill_then_feather_then_at_a_feather_without_a_blend():
    for given, field in (({'blend': 0.0, 'fill': 0.0, 'feather': 0}, 'blend'), ({'blend': 0.5, 'fill': 0.0, 'feather': 0}, 'fill'),
                         ({'fill': 0.0, 'feather': 0}, 'fill'), ({'feather': 0}, 'feather'), ({'blend': 0.5, 'feather': 0}, 'feather')):
        with pytest.raises(ValueError) as e:
            engine.MosaicOptions(**given).checked()
        assert e.value.field == field and str(e.value) == TEXT[field].format(given[field])
    for who, name in (((), 'MosaicOptions'), (('mosaic_of',), 'mosaic_of')):
        with pytest.raises(ValueError) as e:
            engine.MosaicOptions(feather=8, fill=0.5).checked(*who)
        assert str(e.value) == f'{name}: a feather is a factor of the blend\'s weight; give the blend depth too (blend=H)' and e.value.field == 'feather'


def test_checked_looks_at_every_value_in_the_tables_order_and_then_at_the_combinations_in_theirs():
    wrong = {'blend': 0.0, 'fill': 0.0, 'feather': 0, 'bands': 0, 'surface': 0.0, 'support': 0, 'gains': 0, 'gain_limit': 0.0, 'gain_solve': 'exact',
             'reject': 0.0}
    right = {'blend': 0.5, 'fill': 0.1, 'feather': 8, 'bands': 2, 'surface': 0.05, 'support': 2, 'gains': 3, 'gain_limit': 2.0, 'gain_solve': 'direct',
             'reject': 0.15}
    for i, field in enumerate(TABLE):      # every field before it right, it and every field after it wrong: it is the one refused
        given = {**{f: right[f] for f in TABLE[:i]}, **{f: wrong[f] for f in TABLE[i:]}}
        with pytest.raises(ValueError) as e:
            engine.MosaicOptions(**given).checked()
        assert e.value.field == field and str(e.value) == TEXT[field].format(wrong[field]) and e.value.needs is None
    # a bad value of any field is refused before a missing partner of any other
    with pytest.raises(ValueError) as e:
        engine.MosaicOptions(feather=8, reject=0.0).checked()
    assert e.value.field == 'reject' and e.value.needs is None
    with pytest.raises(ValueError) as e:          # the limit's value before the missing rounds
        engine.MosaicOptions(gain_limit=17).checked()
    assert e.value.field == 'gain_limit' and 'within' in str(e.value)
    lone = {f: right[f] for f in NEEDS}           # all five given without what they go with
    order = list(NEEDS)
    partner = {row[0]: row[1] for row in engine.MOSAIC_NEEDS}
    for i, field in enumerate(order):             # the rows before it not asked for: it is the one refused
        given = {f: lone[f] for f in order[i:]}
        for who in ('MosaicOptions', 'Mosaic.begin', 'Mosaic.run', 'mosaic_of', 'mosaic'):
            with pytest.raises(ValueError) as e:
                engine.MosaicOptions(**given).checked(who)
            assert str(e.value) == f'{who}: {NEEDS[field]}' and e.value.field == field and e.value.needs == partner[field]
    assert engine.MosaicOptions(**right).checked() == engine.MosaicOptions(**right).checked().checked()
    # the rejection and the fill go with anything, alone too
    assert engine.MosaicOptions(reject=0.15, fill=0.1).checked() == engine.MosaicOptions(fill=0.1, reject=np.float32(0.15))


REFUSAL = {'blend': '--mosaic-blend: H must be a finite depth within [{:g}, {:g}] metres, not {}',
           'fill': '--mosaic-fill: R must be a finite reach within [{:g}, {:g}] metres, not {}',
           'feather': '--mosaic-feather: F must be an integer within [{:g}, {:g}] source pixels, not {:g}',
           'bands': '--mosaic-bands: K must be an integer within [{:g}, {:g}] bands, not {:g}',
           'surface': '--mosaic-surface: T must be a finite tolerance within [{:g}, {:g}] metres, not {}',
           'support': '--mosaic-support: M must be an integer within [{:g}, {:g}] views, not {:g}',
           'gains': '--mosaic-gains: R must be an integer within [{:g}, {:g}] rounds, not {:g}',
           'gain_limit': '--mosaic-gain-limit: L must be a finite limit within [{:g}, {:g}] times, not {}',
           'reject': '--mosaic-reject: T must be a finite tolerance within [{:g}, {:g}] colour units, not {}'}
HEAD = {'blend': '--mosaic-blend: H must be a finite depth within [1e-06, 1e+06] metres',
        'fill': '--mosaic-fill: R must be a finite reach within [1e-06, 1e+06] metres',
        'feather': '--mosaic-feather: F must be an integer within [1, 1024] source pixels',
        'bands': '--mosaic-bands: K must be an integer within [1, 6] bands',
        'surface': '--mosaic-surface: T must be a finite tolerance within [1e-06, 1e+06] metres',
        'support': '--mosaic-support: M must be an integer within [1, 4] views',
        'gains': '--mosaic-gains: R must be an integer within [1, 64] rounds',
        'gain_limit': '--mosaic-gain-limit: L must be a finite limit within [1, 16] times',
        'reject': '--mosaic-reject: T must be a finite tolerance within [1e-06, 1e+06] colour units'}


@pytest.mark.parametrize('field', NUMBERS)
def test_the_command_line_refuses_with_the_numbers_of_the_table(field):
    lo, hi = engine.MOSAIC_VALUES[field][1]
    assert REFUSAL[field].format(lo, hi, 0.0).split(', not')[0] == HEAD[field]
    for value in (float(lo), float(hi)):
        sucre._refuse_mosaic_values(argparse.Namespace(**{'mosaic_' + field: value}))
    outside = [lo * 0.99, hi * 1.01, NAN, INF] + ([2.5] if engine.MOSAIC_VALUES[field][2] else [])
    for value in outside:
        with pytest.raises(SystemExit) as e:
            sucre._refuse_mosaic_values(argparse.Namespace(**{'mosaic_' + field: value}))
        assert str(e.value.code) == REFUSAL[field].format(lo, hi, value)


def test_the_command_line_refuses_a_solve_that_is_no_choice_and_looks_at_the_flags_in_the_tables_order():
    for value in engine.MOSAIC_GAIN_SOLVES:
        sucre._refuse_mosaic_values(argparse.Namespace(mosaic_gain_solve=value))
    for value in ('exact', 'Direct', '1'):
        with pytest.raises(SystemExit) as e:
            sucre._refuse_mosaic_values(argparse.Namespace(mosaic_gain_solve=value))
        assert str(e.value.code) == f'--mosaic-gain-solve: S must be rounds or direct, not {value}'
    wrong = {'mosaic_' + f: 0.0 for f in NUMBERS}
    wrong['mosaic_gain_solve'] = 'exact'
    for i, field in enumerate(TABLE):
        with pytest.raises(SystemExit) as e:
            sucre._refuse_mosaic_values(argparse.Namespace(**{'mosaic_' + f: wrong['mosaic_' + f] for f in TABLE[i:]}))
        assert str(e.value.code).startswith(sucre._MOSAIC_FLAG[field] + ': ')
    assert sucre._ONLY_WITH[-2:] == [('--mosaic-gain-solve', '--mosaic-gains', 'R'), ('--mosaic-reject', '--mosaic', 'DIR')]
    assert not hasattr(sucre, '_refuse_lone_gain_solve') and not hasattr(sucre, '_refuse_lone_reject')
