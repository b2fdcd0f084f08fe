"""CPU tests of the pure pieces of tests/ftrain_drive.py, the driver of the trainer's GPU tests: the bitwise comparison, the poisoned
padding, the per-tensor step error, the label matrix of the exact fold, the files of the `kws train` tests, and the inputs the GPU
tests feed, pinned by digest: the float64 bounds' preconditions are shown by the *_cpu.py suites on these very inputs."""
import hashlib

import numpy as np
import pytest

import fnet_rows
import ftrain_drive as ftd
import ftrain_rows
from edison_amd import cube_import, train


def test_same_bits_is_bitwise():
    a = np.linspace(-3.0, 3.0, 24, dtype=np.float32).reshape(4, 6)
    assert ftd.same_bits(a, a.copy()) and ftd.same_bits(a[:, ::2], a[:, ::2].copy())
    b = a.copy()
    b.view(np.uint32)[2, 5] ^= 1                      # one mantissa bit
    assert not ftd.same_bits(b, a)
    z = np.zeros(3, np.float32)
    m = z.copy()
    m[1] = -0.0
    assert (m == z).all() and not ftd.same_bits(m, z)
    nan = np.array([0x7fc00001, 0x7fc00001], np.uint32).view(np.float32)
    assert (nan != nan).all() and ftd.same_bits(nan, nan.copy())
    assert not ftd.same_bits(nan, np.array([0x7fc00001, 0x7fc00002], np.uint32).view(np.float32))
    assert not ftd.same_bits(np.zeros(3, np.float32), np.zeros(3, np.float64))                  # dtype
    assert not ftd.same_bits(np.zeros(3, np.int32), np.zeros(3, np.int64))
    assert not ftd.same_bits(np.zeros((3, 1), np.float32), np.zeros(3, np.float32))             # shape


def test_pow2_at_least():
    assert [ftd.pow2_at_least(v) for v in (0, 1, 2, 3, 1024, 1025)] == [1, 1, 2, 4, 1024, 2048]


@pytest.mark.parametrize("name,blob_of", [("pool21_trunc_h", fnet_rows.blob), ("sym3x3", ftrain_rows.pad_blob)])
def test_poisoned_writes_the_padding_and_nothing_else(name, blob_of):
    blob = blob_of(name)
    bad, real = ftd.poisoned(blob)
    model = cube_import.read_blob(blob)
    lay, n = train.layout(model)
    recs = train.conv_records(model)
    assert real.shape == (n,) and real.dtype == bool and 0 < real.sum() < n             # there is padding to poison
    ramp = [dict(w=np.arange(1, L["w"].size + 1, dtype=np.float32).reshape(r["shape"]), b=-np.arange(1, r["out_c"] + 1, dtype=np.float32))
            for L, r in zip(recs, lay)]
    assert np.array_equal(train.pack(ramp, lay) != 0, real)                             # the mask is the real entries of train.pack
    assert int(real.sum()) == sum(L["w"].size + L["b"].size for L in recs)
    w, w0 = np.frombuffer(bad, "<f4", n, len(bad) - 4 * n), np.frombuffer(blob, "<f4", n, len(blob) - 4 * n)
    assert len(bad) == len(blob) and bad[:len(blob) - 4 * n] == blob[:len(blob) - 4 * n]  # the header and the records stay
    assert (w[~real] == np.float32(1.0e6)).all() and ftd.same_bits(w[real], w0[real])
    assert ftd.same_bits(w0[real], train.pack([dict(w=L["w"], b=L["b"]) for L in recs], lay)[real])
    other, real2 = ftd.poisoned(blob, value=-2.5)
    assert np.array_equal(real2, real) and (np.frombuffer(other, "<f4", n, len(blob) - 4 * n)[~real] == np.float32(-2.5)).all()
    m, cached, real3 = ftd.case(name)
    assert cached == bad and np.array_equal(real3, real) and ftd.case(name)[1] is cached   # built once


def test_step_errors_normalise_per_tensor_and_skip_the_padding():
    # two records: w [k_pad 2][n_pad 4] + b [4] at 0, w [k_pad 1][n_pad 2] + b [2] at 12; the last column of record 0 is padding
    layout = [dict(w_at=0, k_pad=2, n_pad=4), dict(w_at=12, k_pad=1, n_pad=2)]
    assert list(ftd.tensors(layout)) == [(0, 8), (8, 12), (12, 14), (14, 16)]
    real = np.ones(16, bool)
    real[[3, 7, 11]] = False
    want = np.array([1, 2, 4, 1e6, -8, 2, 1, 1e6, 0.5, 0.25, 0.5, 1e6, 100, -50, 0.001, 0.002])
    got = want.copy()
    got[[0, 4]] += 0.5                # tensor maximum 8
    got[9] += 0.125                   # 0.5
    got[13] += 1.0                    # 100
    got[14] -= 0.001                  # 0.002
    got[[3, 7, 11]] = 7.0             # the padding is not looked at, however wrong
    err = ftd.step_errors(layout, real, got, want)
    expect = np.zeros(16)
    expect[[0, 4]], expect[9], expect[13], expect[14] = 0.5 / 8, 0.125 / 0.5, 1.0 / 100, 0.001 / 0.002
    assert np.allclose(err, expect, rtol=1e-12, atol=0) and not err[~real].any()


def test_tile_labels_put_a_tiles_own_labels_first_and_fillers_behind():
    b, N, n1 = 3, 8, 4
    y = (np.arange(N + n1) % 5).astype(np.int32)
    labels = ftd.tile_labels(y[:N], b, n1)
    assert labels.dtype == np.int32 and labels.tolist() == [[0, 1, 2, -1], [3, 4, 0, -1], [1, 2, -1, -1]]
    n_tiles = (N + b - 1) // b
    assert labels.shape == (n_tiles, n1) and int((labels < 0).sum()) == n_tiles * n1 - N
    assert int((labels[0] < 0).sum()) == n1 - b                                         # what the ignored counter shows after tile 0


def _digest(x, y):
    assert x.dtype == np.float32 and y.dtype == np.int32 and len(x) == len(y)
    return hashlib.sha256(x.tobytes() + y.tobytes()).hexdigest()


# SHA-256 of rows + labels as test_gpu_ftrain.data, test_gpu_ftrain_tiles.rows and test_gpu_ftrain_pad's fold test drew them before
# they moved to the driver
DATA = {("pool21_trunc_h", 17): "270fa5dc65d1eeef6d2506c599b8081a2e6710f4e7e06c37f0eb6d89945154c6",
        ("relu_logits", 5): "fa341cb79a584018cff927dd989d508500fd45635257e7c2931fad2d1b7126bb",
        ("cube_kws", 9): "71a5585fd713899d41b7da5a49da1163d5762e38e0e5e6d4e322125662938a88"}
ROWS_EXACT = {("pool21_trunc_h", 6): "82232e50cbb33ad60efde7bf04d16430d5cde47266144a388cafb6b199eaffe5",
              ("cube_kws", 6): "7b60acc5af0095691e383659e55b4f1d0f571f8fed43bd1b0378f2433b242440",
              ("sym3x3", 12): "71ca8ed990335ad8b04677bce8007fadeaba30991faefec491bb2ba10fece6a1"}      # the padded fold's draw


@pytest.mark.parametrize("name,n", sorted(DATA))
def test_data_did_not_move(name, n):
    model = ftd.case(name)[0]
    x, y = ftd.data(name, model, n)
    assert x.shape == (n, int(np.prod(model["in_shape"]))) and _digest(x, y) == DATA[name, n]
    if name == "relu_logits":
        assert (x < 0).all()


@pytest.mark.parametrize("name,n", sorted(ROWS_EXACT))
def test_rows_did_not_move_and_a_shorter_draw_is_a_prefix(name, n, monkeypatch):
    model = ftd.case(name)[0]
    drawn = {}
    for exact in (True, False) if name in fnet_rows.SWEEP or name == "cube_kws" else (True,):      # data draws sweep rows only
        monkeypatch.setattr(ftd, "_ROWS", {})                                            # a cache of this test's own
        x, y = drawn[exact] = ftd.rows(name, model, n, exact=exact)
        if exact:
            assert _digest(x, y) == ROWS_EXACT[name, n]
        held = ftd._ROWS[name, exact]
        assert np.shares_memory(ftd.rows(name, model, n - 1, exact=exact)[0], held[0])  # a shorter draw does not draw again
        x2, y2 = ftd.rows(name, model, 2 * n, exact=exact)                              # a longer one does, and the old one is its prefix
        assert len(y2) == 2 * n and ftd.same_bits(x2[:n], x) and np.array_equal(y2[:n], y)
        assert ftd._ROWS[name, exact] is not held and np.shares_memory(ftd.rows(name, model, n, exact=exact)[0], x2)
    assert len(drawn) == 1 or not ftd.same_bits(drawn[True][0], drawn[False][0])


def test_kws_files_writes_what_the_readers_read(tmp_path):
    model = fnet_rows.model(ftrain_rows.FIT_ROW)
    x, y = ftrain_rows.fit_set()
    args, val = ftd.kws_files(tmp_path, model, x, y, ["a", "b", "c"])
    assert args == [str(tmp_path / "net.ednf"), str(tmp_path / "x.npy"), str(tmp_path / "y.npy")] and val == (args[1], args[2])
    assert ftd.same_bits(np.load(args[1]), x) and ftd.same_bits(np.load(args[2]), y)
    with open(args[0], "rb") as f:
        back = cube_import.read_blob(f.read())
    assert back["keywords"] == ["a", "b", "c"] and tuple(back["in_shape"]) == tuple(model["in_shape"])
    for a, b in zip(train.conv_records(back), train.conv_records(model)):
        assert ftd.same_bits(a["w"], b["w"]) and ftd.same_bits(a["b"], b["b"])
    audio = ftd.kws_audio(11 * 1024)
    assert audio.shape == (6, 11264) and audio.dtype == np.int16 and np.array_equal(audio, ftd.kws_audio(11 * 1024))
    assert ftd.fit_kw() == dict(epochs=100, batch_size=32, seed=0, lr=0.01, max_steps=40)
