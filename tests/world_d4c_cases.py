"""What the D4C tests (tests/test_world_d4c_*.py) and the tolerance measurement (scripts/d4c_tolerance.py) share beside the inputs of
tests/world_analysis_cases.py: the seed of the noise term and the bars read from profiles/r10/d4c_tolerance.txt.

SEED: on the `zeros` / `click` / `short` waves the Love-Train ratio a0 is made by the noise term alone, so whether a frame lands within 1e-6 of
the threshold depends on the seed; tests/test_world_d4c_ref.py holds every voiced frame of the case set to |a0 - 0.85| >= 1e-6 with this seed."""
from pathlib import Path

SEED = 5
MARGIN = 1e-6
ROOT = Path(__file__).resolve().parent.parent


def bars():
    """(a0, coarse dB, ap dB): 4 x the float64-vs-longdouble figures of the restatement (lines 1 to 3 of profiles/r10/d4c_tolerance.txt)."""
    lines = (ROOT / 'profiles' / 'r10' / 'd4c_tolerance.txt').read_text().splitlines()
    assert lines[0].startswith('worst a0') and lines[1].startswith('worst coarse') and lines[2].startswith('worst ap')
    return tuple(4 * float(lines[i].split()[-1]) for i in range(3))
