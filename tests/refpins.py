"""Outputs of the reference's own compiled code (oracle/_ref: built by oracle/Makefile only where the reference's sources are at hand),
recorded in tests/golden/refpins_golden.npz by tests/golden/gen_fixtures_refpins.py, so that the tests pinned to that code hold on a
machine without it. With oracle/_ref present a test computes the reference's outputs live AND checks the recording against them;
without it, the test takes the recording.

Outputs too large to store (whole transforms of ~16 k frames) are recorded as SHA-256 digests of their values: `digests()`."""
import hashlib
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpins_golden.npz")
RECORD = None   # tests/golden/gen_fixtures_refpins.py sets a dict here: live outputs are collected into it instead of checked
_golden = None


def _recorded():
    global _golden
    if _golden is None:
        with np.load(PATH) as g:
            _golden = {k: g[k] for k in g.files}
    return _golden


def digest(a):
    """SHA-256 of an array's shape and values (integers by value whatever their width, floats by bit pattern), hex."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        a = a.view(np.dtype("u%d" % a.dtype.itemsize))
    h = hashlib.sha256(repr(tuple(a.shape)).encode())
    h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
    return h.hexdigest()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _take(key, live, conv):
    """live: a callable returning {name: array} from the reference's code, or None where that code is absent here."""
    if live is None:
        g = _recorded()
        out = {k.split("/", 1)[1]: v for k, v in g.items() if k.split("/", 1)[0] == key}
        assert out, "%s is not recorded in %s (tests/golden/gen_fixtures_refpins.py writes it)" % (key, PATH)
        return out
    out = {name: conv(np.asarray(v)) for name, v in live().items()}
    if RECORD is not None:
        RECORD.update({key + "/" + name: v for name, v in out.items()})
        return out
    g = _recorded()
    for name, v in out.items():
        assert key + "/" + name in g and _same(g[key + "/" + name], v), \
            "the reference's %s/%s differs from its recording in %s: regenerate it (tests/golden/gen_fixtures_refpins.py)" % (key, name, PATH)
    return out


def outputs(key, live):
    """{name: array}: the reference's outputs, live or recorded."""
    return _take(key, live, np.ascontiguousarray)


def digests(key, live):
    """{name: hex digest} of the reference's outputs, live or recorded (compare with digest() of what is checked)."""
    return {name: str(v) for name, v in _take(key, live, lambda a: np.array(digest(a))).items()}
