"""Vectors recorded from the reference project's own code, for the tests that compare against it without needing it at run time.

usage: RY_REFERENCE_DIR=<checkout of the reference project> python tests/golden/make_reference_goldens.py

-> tests/golden/reference/vocoder_decode.npz: `RealtimeVocoder.decode` (yukarin_wrapper/vocoder.py) called four times on one vocoder
   object over the recording world4py stand-in (tests/world4py_fake.py), for the float64 features test_vocoder_feed.feature(100, seed),
   seed 0..3: wave0..wave3 and sampling_rate (tests/test_vocoder_feed.py)."""
import importlib
import sys
from pathlib import Path

import numpy
import pytest

ROOT = Path(__file__).resolve().parents[2]
OUT = ROOT / 'tests' / 'golden' / 'reference'


def main():
    sys.path[:0] = [str(ROOT), str(ROOT / 'tests'), str(ROOT / 'tests' / 'stubs')]
    import reference_checkout
    ref = reference_checkout.reference_dir()
    if ref is None:
        raise SystemExit('set RY_REFERENCE_DIR to a checkout of the reference project')
    sys.path.insert(0, str(ref))
    import test_vocoder_feed as tv
    import world4py_fake
    mp = pytest.MonkeyPatch()
    try:
        world4py_fake.install(mp)
        voc = importlib.import_module('realtime_voice_conversion.yukarin_wrapper.vocoder')
        v = voc.RealtimeVocoder.__new__(voc.RealtimeVocoder)
        v._synthesizer = world4py_fake.WorldSynthesizer()
        v._before_buffer = []
        v.out_sampling_rate = 24000
        waves = [voc.RealtimeVocoder.decode(v, tv.feature(100, s, numpy.float64)) for s in range(4)]
    finally:
        mp.undo()
    assert len(set(w.sampling_rate for w in waves)) == 1
    OUT.mkdir(parents=True, exist_ok=True)
    numpy.savez_compressed(str(OUT / 'vocoder_decode.npz'), sampling_rate=numpy.int64(waves[0].sampling_rate),
                           **{'wave%d' % i: numpy.asarray(w.wave, numpy.float64) for i, w in enumerate(waves)})
    print('wrote', OUT / 'vocoder_decode.npz')


if __name__ == '__main__':
    main()
