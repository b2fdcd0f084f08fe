"""CPU tests of the pure pieces of tests/stream_drive.py, the driver of the stream and bank tests: the bitwise comparison, the comparison
of a bank with its streams, the schedules, the numpy filter against the oracle's C restatement, the recordings (pinned by digest: the
GPU tests' rows depend on the exact samples) and the option plumbing of Kind."""
import hashlib

import numpy as np
import pytest

import stream_drive as sd
from geom_sweep import GEOMS, geom


def _fails(call, *words):
    with pytest.raises(AssertionError) as e:
        call()
    assert all(w in str(e.value) for w in words), str(e.value)


def test_same_is_bitwise():
    a = np.linspace(-3.0, 3.0, 24, dtype=np.float32).reshape(4, 6)
    sd.same(a, a.copy(), "equal")
    sd.same(np.arange(5, dtype=np.int8), np.arange(5, dtype=np.int8), "equal int8")
    b = a.copy()
    b.view(np.uint32)[2, 5] ^= 1                      # one mantissa bit
    _fails(lambda: sd.same(b, a, "flipped"), "flipped", "1 of 24", "(2, 5)")
    z = np.zeros(3, np.float32)
    m = z.copy()
    m[1] = -0.0
    assert (m == z).all()
    _fails(lambda: sd.same(m, z, "zeros"), "(1,)")
    nan = np.array([0x7fc00001, 0x7fc00001], np.uint32).view(np.float32)
    assert (nan != nan).all()
    sd.same(nan, nan.copy(), "equal NaN bit patterns")
    _fails(lambda: sd.same(nan, np.array([0x7fc00001, 0x7fc00002], np.uint32).view(np.float32), "payload"), "(1,)")
    _fails(lambda: sd.same(np.zeros(3, np.int32), np.zeros(3, np.int64), "dtype"), "dtype")
    _fails(lambda: sd.same(np.zeros((3, 1), np.int32), np.zeros(3, np.int32), "shape"), "shape")


@pytest.mark.parametrize("kind", ["int8", "float"])
def test_same_as_streams(kind):
    K = sd.Kind(kind)
    rng = np.random.default_rng(4)
    rows, M, no = 6, 3, 10

    def stream():
        o = {"logits": rng.integers(-100, 100, (rows, no)).astype(K.dtype), K.second: rng.integers(0, 100, (rows, no)).astype(K.dtype),
             "argmax": rng.integers(0, no, rows).astype(np.int32), "filtered": rng.random((rows, no)).astype(np.float32),
             "likely": rng.integers(0, no, rows).astype(np.int32), "spotted": rng.integers(-1, no, rows).astype(np.int32)}
        return o

    ref = [stream() for _ in range(M)]
    bank = lambda: {k: np.stack([r[k] for r in ref], axis=1) for k in ref[0]}
    sd.same_as_streams(K, bank(), ref, "equal")
    got = bank()
    got["likely"].view(np.uint8).reshape(rows, M, 4)[4, 2, 1] ^= 0x40          # one byte of microphone 2's likely, row 4
    _fails(lambda: sd.same_as_streams(K, got, ref, "a byte"), "a byte microphone 2 likely", "(4,)")
    sd.same_as_streams(K, got, ref, "the others", mics=(0, 1))
    sd.same_as_streams(K, {k: v[2:4] for k, v in bank().items()}, [{k: v[2:4] for k, v in r.items()} for r in ref], "rows")
    got = dict(bank(), fsm_states=np.zeros((rows, M), np.int32))            # an output the reference does not have
    _fails(lambda: sd.same_as_streams(K, got, ref, "extra key"), "extra key", "fsm_states")
    none = [dict(r, **{K.second: None}) for r in ref]                         # a graph without a second output
    sd.same_as_streams(K, dict(bank(), **{K.second: None}), none, "no second output")
    _fails(lambda: sd.same_as_streams(K, bank(), none, "second output on one side"), K.second)


def test_schedules():
    assert sd.schedule(3, 24) == [3, 3, 1, 3, 3, 3, 1, 3, 3, 3, 1, 3, 3, 3, 1, 3, 3, 3, 1, 3, 3, 3, 1, 3]
    assert sd.schedule(3, 30, sd.by_round) == [3, 3, 1, 3, 3, 3, 2, 3, 3, 3, 1, 3, 3, 3, 2, 3, 3, 3, 1, 3, 3, 3, 2, 3, 3, 3, 1, 3, 3, 3]
    assert sd.schedule(3, 30, None) == [3] * 30
    for ragged in (sd.by_push, sd.by_round, None):
        assert sd.schedule(1, 30, ragged) == [1] * 30                         # chunk 1 has no ragged push
    assert sd.schedule(5, 12, sd.by_push) == [5, 5, 3, 5, 5, 5, 3, 5, 5, 5, 3, 5] and sd.schedule(5, 12, sd.by_round)[2::4] == [1, 2, 3]
    assert sd.wraps([1] * 30, 1) == [8, 16, 24] and len(sd.wraps(sd.schedule(1, 30, sd.by_round), 1, slots=8)) >= 3
    assert sd.wraps(sd.schedule(3, 30, sd.by_round), 3) == [9, 18, 27] and sd.wraps(sd.schedule(3, 24), 3) == [9, 19]
    assert sd.wraps([3] * 8, 3) == [] and sd.wraps([3] * 9, 3) == [8]
    assert sd.whole(300, 7) == [7] * 42 + [6] and sd.whole(14, 7) == [7, 7] and sd.whole(3, 512) == [3]


@pytest.mark.parametrize("alpha,threshold", [(0.9, 0.5), (0.5, 0.5), (0.6, 3.0), (0.0, 80.0), (0.999, 0.0)])
def test_filter_ref_equals_the_oracle(oracle_mod, alpha, threshold):
    """The numpy filter the GPU tests use against oracle/postproc_ref.c's, bit for bit, on 4 000 seeded int8 rows of 10 classes."""
    x = np.random.default_rng(1).integers(-128, 128, (4000, 10)).astype(np.int8)
    filt, likely, spotted = sd.filter_ref(x, alpha, threshold)
    want = oracle_mod.output_filter(x, alpha=alpha, threshold=threshold)
    sd.same(filt, want[0], "filtered")
    sd.same(likely, want[1], "likely")
    sd.same(spotted, want[2], "spotted")
    assert (spotted >= 0).any() and (spotted < 0).any()


# SHA-256 of the arrays the functions gave in test_gpu_stream_bank / test_gpu_stream_geom before they moved to the driver
RECORDINGS = "827a788a6d7e0d714eecb60f2f6c1ec06c38e39194b91600e5a17d34bde9f79d"
RECORDING = "cde40f1b323ccc92a0033eab93b416f8e220da826ac595154e0be4bd2e88ac31"


def test_recordings_did_not_move():
    g = geom(**GEOMS["square"])
    x = sd.recordings(g, 3, 24, 103)
    assert x.shape == (3, 24 * g.frame_step) and x.dtype == np.int16
    assert hashlib.sha256(x.tobytes()).hexdigest() == RECORDINGS
    assert np.array_equal(x, sd.recordings(g, 3, 24, 103))
    assert not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2]) and not np.array_equal(x[0], x[2])
    y = sd.recording(geom(), 300, 14)
    assert y.shape == (300 * 1024,) and y.dtype == np.int16
    assert hashlib.sha256(y.tobytes()).hexdigest() == RECORDING
    assert np.array_equal(y, sd.recording(geom(), 300, 14)) and not np.array_equal(y, sd.recording(geom(), 300, 15))
    assert sd.tail(g) == 240 and sd.tail(geom(**GEOMS["kws_small"])) == 0


def test_kind_keys():
    assert tuple(sd.Kind("int8").keys(True, True)) == ("logits", "softmax", "argmax", "filtered", "likely", "spotted", "fsm_states")
    assert tuple(sd.Kind("float").keys(True, True)) == ("logits", "probs", "argmax", "filtered", "likely", "spotted", "fsm_states")
    K = sd.Kind("int8")
    K.has_second = False
    assert K.keys(True, False) == ["logits", "argmax", "filtered", "likely", "spotted"] and K.keys(False, False) == ["logits", "argmax"]
    assert sd.Kind("float").keys(False, False) == ["logits", "probs", "argmax"]
    assert (sd.Kind("int8").dtype, sd.Kind("float").dtype) == (np.int8, np.float32)


def test_kind_passes_the_options_on(monkeypatch):
    """The constructors differ (FloatBank(c, M, g, q15=) against StreamBank(c, g, M)); Kind hides that and nothing else."""
    from edison_amd import stream
    calls = []

    def fake(name):
        return lambda *a, **kw: calls.append((name, a, kw))

    for name in ("GeomStream", "StreamBank", "FloatStream", "FloatBank"):
        monkeypatch.setattr(stream, name, fake(name))
    K = sd.Kind("int8")
    K.stream("c", "g", 7, output_filter=True, alpha=None, threshold=3.0, fsm=False)
    K.bank("c", "g", 5, 3, output_filter=True, alpha=0.6, threshold=None, fsm=True)
    F = sd.Kind("float", q15=True)
    F.stream("c", "g", 7, output_filter=False, alpha=None, threshold=None)
    F.bank("c", "g", 5, 3, fsm=True, q15=False, clip_min=-1.0, clip_max=1.0)
    assert calls == [("GeomStream", ("c", "g"), dict(chunk_frames=7, output_filter=True, threshold=3.0, fsm=False)),
                     ("StreamBank", ("c", "g", 5), dict(chunk_frames=3, output_filter=True, alpha=0.6, fsm=True)),
                     ("FloatStream", ("c", "g"), dict(chunk_frames=7, output_filter=False, q15=True)),
                     ("FloatBank", ("c", 5, "g"), dict(chunk_frames=3, fsm=True, q15=False, clip_min=-1.0, clip_max=1.0))]
