"""Every refusal of the command line, replayed: tests/golden/cli_refusals.json holds, for each of the 18 flags that some mode
refuses or that take a value check, alone and in every unordered pair, and for the bad values, what ``sucre.main`` answers on
directories that do not exist -- the exact ``SystemExit`` text, or ``accepted`` when the run gets as far as looking for the
model.  Recorded before the refusal tables were merged into one (``PYTHONPATH=. python tests/test_cli_refusals.py`` from the
repository's root writes the file anew from the code it is run on); the test compares strings for equality and leaves no
case out.  No GPU."""
import itertools
import json
from pathlib import Path

import pytest

from sucre_amd import sucre

GOLDEN = Path(__file__).parent / 'golden' / 'cli_refusals.json'
BASE = ['--image-dir', 'i', '--depth-dir', 'd', '--model-dir', 'm', '--output-dir', 'o', '--image-name', 'x.png']   # test_trim_host.py's
FLAGS = [['--shared-water'], ['--save-quality'], ['--trim-outliers', '3'], ['--trim-rounds', '2'], ['--view-gains'],
         ['--gain-rounds', '2'], ['--gain-limit', '1.5'], ['--apply-water', 'nowhere/water.pt'], ['--check-consistency', 'results'],
         ['--mosaic', 'results'], ['--mosaic-gsd', '0.1'], ['--mosaic-blend', '0.5'], ['--common-stretch'],
         ['--stretch-from', 'nowhere/stretch.pt'], ['--save-interval', '5'], ['--params-path', 'nowhere/params.pt'],
         ['--keep-matches'], ['--image-scale', '0.5']]
BAD_VALUES = [['--trim-outliers', '0'], ['--trim-outliers', 'nan'], ['--trim-outliers', '3', '--trim-rounds', '0'],
              ['--view-gains', '--gain-rounds', '0'], ['--view-gains', '--gain-limit', '0.9'], ['--mosaic', 'results', '--mosaic-gsd', '0'],
              ['--mosaic', 'results', '--mosaic-blend', 'inf']]


def cases() -> list:
    return [f for f in FLAGS] + [a + b for a, b in itertools.combinations(FLAGS, 2)] + BAD_VALUES


def outcome(extra: list) -> str:
    try:
        sucre.main(BASE + extra)
    except SystemExit as e:
        assert isinstance(e.code, str), (extra, e.code)   # (argparse's own exits carry a number: none is expected here)
        return e.code
    except FileNotFoundError as e:
        assert Path(e.filename).parts[0] == 'm', (extra, e)   # the model directory: nothing was refused
        return 'accepted'
    raise AssertionError(f'{extra}: the run neither refused nor looked for the model')


def test_every_recorded_answer_is_given_again(monkeypatch, capsys):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    recorded = json.loads(GOLDEN.read_text())
    assert [r['argv'] for r in recorded] == cases() and len(recorded) == 18 + 153 + 7
    assert sum(r['outcome'] == 'accepted' for r in recorded) == 37
    for r in recorded:
        assert outcome(r['argv']) == r['outcome'], r['argv']


if __name__ == '__main__':
    import os
    os.environ.pop('WORLD_SIZE', None)
    GOLDEN.write_text(json.dumps([{'argv': c, 'outcome': outcome(c)} for c in cases()], indent=0) + '\n')
