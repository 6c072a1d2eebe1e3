"""Host tests of ``engine.MosaicOptions``: ``checked()`` against the three public validators on the ends of every range, and the
numbers of the command line's refusals against ``engine.MOSAIC_VALUES``.  No GPU."""
import argparse
import dataclasses

import numpy as np
import pytest

from sucre_amd import engine, sucre

NAN, INF = float('nan'), float('inf')
VALIDATOR = {'blend': engine.mosaic_blend_depth, 'fill': engine.mosaic_fill_reach, 'feather': engine.mosaic_feather_px}
KIND = {'blend': np.float32, 'fill': float, 'feather': int}
GOOD = {'blend': [1e-6, 1e6, 0.5, '0.5', np.float32(2)], 'fill': [1e-6, 1e6, 0.05, '3', np.float64(2)], 'feather': [1, 1024, 8.0, '16', np.int64(3)]}
BAD = {'blend': [9.9e-7, 1.0000001e6, 0.0, -1.0, NAN, INF, -INF, 'deep'],
       'fill': [9.9e-7, 1.0000001e6, 0.0, -1.0, NAN, INF, -INF, 'far'],
       'feather': [0, 1025, -3, NAN, INF, True, False, 2.5, 1.5, 'wide']}
TEXT = {'blend': 'mosaic blend depth H must be finite and within [1e-06, 1e+06] metres, not {}',
        'fill': 'mosaic fill reach R must be finite and within [1e-06, 1e+06] metres, not {}',
        'feather': 'mosaic feather width F must be an integer within [1, 1024] source pixels, not {}'}


def options(field, value):
    """The record with ``value`` in ``field`` -- and a blend next to a feather, which needs one."""
    return engine.MosaicOptions(**{'blend': 0.5} if field == 'feather' else {}, **{field: value})


def test_the_table_holds_the_public_ranges():
    assert list(engine.MOSAIC_VALUES) == ['blend', 'fill', 'feather']      # the order in which checked() looks at them
    assert [f.name for f in dataclasses.fields(engine.MosaicOptions)] == ['blend', 'feather', 'fill']
    assert engine.MOSAIC_VALUES['blend'][1] is engine.MOSAIC_BLEND_RANGE and engine.MOSAIC_BLEND_RANGE == (1e-6, 1e6)
    assert engine.MOSAIC_VALUES['fill'][1] is engine.MOSAIC_FILL_RANGE and engine.MOSAIC_FILL_RANGE == (1e-6, 1e6)
    assert engine.MOSAIC_VALUES['feather'][1] is engine.MOSAIC_FEATHER_RANGE and engine.MOSAIC_FEATHER_RANGE == (1, 1024)
    assert engine.MosaicOptions() == engine.MosaicOptions(None, None, None) == engine.MosaicOptions().checked()
    with pytest.raises(dataclasses.FrozenInstanceError):
        engine.MosaicOptions().blend = 1.0


@pytest.mark.parametrize('field', ['blend', 'fill', 'feather'])
def test_checked_takes_what_the_validator_takes_and_returns_its_type(field):
    for value in GOOD[field]:
        want = VALIDATOR[field](value)
        got = getattr(options(field, value).checked(), field)
        assert type(want) is KIND[field] and type(got) is KIND[field] and got == want == KIND[field](float(value)), value
        assert options(field, value).checked().checked() == options(field, value).checked()      # at the ends of the range too
    both = engine.MosaicOptions(blend='0.25', feather=4.0, fill=np.float32(0.5)).checked()
    assert (both.blend, both.feather, both.fill) == (np.float32(0.25), 4, 0.5)
    assert [type(x) for x in (both.blend, both.feather, both.fill)] == [np.float32, int, float]
    assert both.checked() == both


@pytest.mark.parametrize('field', ['blend', 'fill', 'feather'])
def test_checked_refuses_what_the_validator_refuses_with_its_text(field):
    for value in BAD[field] + [None]:
        with pytest.raises(ValueError) as want:
            VALIDATOR[field](value)
        assert str(want.value) == TEXT[field].format(value)
        if value is None:      # in the record: not asked for
            continue
        with pytest.raises(ValueError) as got:
            options(field, value).checked()
        assert str(got.value) == str(want.value) and got.value.field == field == want.value.field


@pytest.mark.parametrize('field', ['blend', 'fill'])
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
    so does a float32 reach, which is not the type of a checked reach."""
    low = np.float32(1e-6)
    assert float(low) < 1e-6 and engine.mosaic_blend_depth(low) == low and type(engine.mosaic_blend_depth(low)) is np.float32
    once = engine.MosaicOptions(blend=1e-6).checked()
    assert type(once.blend) is np.float32 and once.checked() == once
    assert engine.mosaic_blend_depth(np.float32(1e6)) == np.float32(1e6)
    for bad in (float(low), np.float64(low), np.nextafter(low, np.float32(0)), np.nextafter(np.float32(1e6), np.float32(np.inf))):
        with pytest.raises(ValueError, match='blend depth H'):
            engine.mosaic_blend_depth(bad)
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


REFUSAL = {'blend': '--mosaic-blend: H must be a finite depth within [{:g}, {:g}] metres, not {}',
           'fill': '--mosaic-fill: R must be a finite reach within [{:g}, {:g}] metres, not {}',
           'feather': '--mosaic-feather: F must be an integer within [{:g}, {:g}] source pixels, not {:g}'}


@pytest.mark.parametrize('field', ['blend', 'fill', 'feather'])
def test_the_command_line_refuses_with_the_numbers_of_the_table(field):
    lo, hi = engine.MOSAIC_VALUES[field][1]
    assert REFUSAL[field].format(lo, hi, 0.0).split(', not')[0] == {
        'blend': '--mosaic-blend: H must be a finite depth within [1e-06, 1e+06] metres',
        'fill': '--mosaic-fill: R must be a finite reach within [1e-06, 1e+06] metres',
        'feather': '--mosaic-feather: F must be an integer within [1, 1024] source pixels'}[field]
    for value in (float(lo), float(hi)):
        sucre._refuse_mosaic_values(argparse.Namespace(**{'mosaic_' + field: value}))
    outside = [lo * 0.99, hi * 1.01, NAN, INF] + ([2.5] if field == 'feather' else [])
    for value in outside:
        with pytest.raises(SystemExit) as e:
            sucre._refuse_mosaic_values(argparse.Namespace(**{'mosaic_' + field: value}))
        assert str(e.value.code) == REFUSAL[field].format(lo, hi, value)
