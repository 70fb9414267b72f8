"""Where the reference project's own checkout is, for the few tests that run its code unchanged on top of the shims.  The reference is
not part of this repository and may not be copied into it.  Each such test module names the checkout's usual location; `RY_REFERENCE_DIR`
overrides it.  `locate()` never raises: a location this user may not read (a parent directory without search permission) counts as
absent, and the tests that need it skip instead of failing the whole module at collection.  What can be checked without the reference's
code is checked against vectors recorded from it (tests/golden/reference/, written by tests/golden/make_reference_goldens.py)."""
import os
from pathlib import Path

SKIP_REASON = 'needs a readable checkout of the reference project (its usual location, or RY_REFERENCE_DIR)'


def locate(default):
    """The reference checkout: RY_REFERENCE_DIR if set, else `default`; None when that directory cannot be read."""
    p = os.environ.get('RY_REFERENCE_DIR') or default
    if not p:
        return None
    try:
        p = Path(p).resolve()
        if (p / 'realtime_voice_conversion').is_dir() and os.access(str(p), os.R_OK | os.X_OK):
            return p
    except OSError:
        pass
    return None


def reference_dir():
    """RY_REFERENCE_DIR alone (the golden writer: it has no usual location of its own)."""
    return locate(None)
