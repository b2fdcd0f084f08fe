"""GPU tests (-m gpu) of calibrating and quantising a float32 network (edison_fcal_*, Context.calibrator / Context.quantize; DESIGN.md
section 18). The reference is stats in tests/fnet_host.py, the host restatement of the statistic on its bit-exact f32 chain: absmax,
the exponent histogram and the count are integers, so every comparison is for equality.

The sweep networks are rows of tests/fnet_rows.py, altered so that each catches one mistake of a calibration kernel:
  pad_rows_big_bias   24 rows per utterance and a bias of 40: at odd utterance counts the last M tile has padding rows, which compute
                      utterance 0's first window again; counting them moves hist and count (absmax only repeats a value it has)
  pad_channels        17 and 4 channels with 1e6 in the blob's bias padding: a counted padding channel is 1e6
  neg_bias_relu       a bias of -30 under ReLU: every output is 0 after it, a statistic taken there is all zero
  trunc_pool_no_relu  pool (1, 2) over 9 columns, conv without ReLU: the dropped column is not counted, negative values are
  batch1              K = 2240 x 16 weights: the calibrator's workgroup holds one utterance
(the others run at batch 16; the shipped network at 7); batch1_lds_max, which fills the LDS to 192 bytes, has no room for the histogram and is refused."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN

import fnet_host as fh
import fnet_plan as fpl
import fnet_rows as fr
from edison_amd import cube_import
from edison_amd import quantize as qz
from oracle import net_ref

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "cube_kws.ednf")
with open(FIXTURE, "rb") as _f:
    SHIPPED_BATCH = fpl.plan(_f.read())["batch"]      # 7: the calibrator's too, the histogram fits in the plan's slack
N_SHIPPED = 3 * SHIPPED_BATCH + 2


@pytest.fixture(scope="module")
def ctx(built_lib):
    from edison_amd.context import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "cube_golden.npz"))


def _fixture_rows(golden):
    return np.stack([golden["net_in_" + str(n)] for n in golden["names"]])


@pytest.fixture(scope="module")
def shipped(golden):
    """The shipped network, 3 batch + 2 inputs (the five fixture rows, then scaled and perturbed copies) and the reference statistic of every
    single input: the statistic of any set of them is the merge."""
    m = fh.load(FIXTURE)
    rows = _fixture_rows(golden)
    rng = np.random.default_rng(18)
    extra = [rows[i % 5] * rng.uniform(0.25, 2.0) + rng.normal(0, 8.0, rows.shape[1]) for i in range(N_SHIPPED - 5)]
    x = np.concatenate([rows, np.array(extra)]).astype(np.float32)
    return m, x, [fh.stats(m, x[i:i + 1]) for i in range(len(x))]


def _merged(per, lo, hi):
    s = per[lo]
    for t in per[lo + 1:hi]:
        s = fh.merge(s, t)
    return s


def _same(got, want, what):
    for k in ("count", "absmax", "hist"):
        assert np.array_equal(got[k], want[k]), "%s: %s differs at index %s" % (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


def test_shipped_network_stats_bit_equal(ctx, shipped):
    m, x, per = shipped
    ctx.fnet_load(FIXTURE)
    with ctx.calibrator() as cal:
        batch = cal.batch
        assert batch == ctx.fnet_info()["batch"] == SHIPPED_BATCH and cal.n_stats == 6 and cal.in_n == 403
        assert cal.info()["lds_bytes"] == ctx.fnet_info()["lds_bytes"] + 4 * 257 <= 160 * 1024
        for n in (1, batch - 1, batch, batch + 1, 3 * batch + 2):
            cal.reset()
            cal.add(x[:n])
            got = cal.result()
            _same(got, _merged(per, 0, n), "n = %d" % n)
            assert (got["hist"].sum(axis=1) == got["count"]).all()
            assert got["count"].tolist() == [n * c for c in (403, 13 * 9 * 2 * 16, 5 * 7 * 2 * 32, 3 * 5 * 64, 1 * 3 * 32, 10)]


def test_adds_accumulate_and_reset_clears(ctx, shipped):
    m, x, per = shipped
    ctx.fnet_load(FIXTURE)
    with ctx.calibrator() as cal:
        cal.add(x[:6])
        cal.add(x[6:20])
        two = cal.result()
        _same(two, _merged(per, 0, 20), "two adds")
        cal.add(x[:0])                                      # nothing
        _same(cal.result(), two, "an empty add")
        cal.reset()
        zero = cal.result()
        assert not zero["absmax"].any() and not zero["hist"].any() and not zero["count"].any()
        cal.add(x[:20])
        _same(cal.result(), two, "one add of the concatenation")


def test_device_add_follows_on_the_stream(ctx, shipped):
    torch = pytest.importorskip("torch")
    m, x, per = shipped
    ctx.fnet_load(FIXTURE)
    dev = torch.device("cuda", 0)
    xt = torch.from_numpy(x).to(dev)
    ctx.use_torch_stream()
    try:
        with ctx.calibrator() as cal:
            cal.add_t(xt[:10], 10)
            cal.add_t(xt[10:], len(x) - 10)
            _same(cal.result(), _merged(per, 0, len(x)), "add_t")
    finally:
        ctx.use_own_stream()


def test_network_outputs_untouched_by_a_calibration(ctx, shipped):
    m, x, per = shipped
    ctx.fnet_load(FIXTURE)
    before, acts = ctx.fnet(x), ctx.fnet_layers(x[:5])
    with ctx.calibrator() as cal:
        cal.add(x)
        during = ctx.fnet(x)
        cal.result()
    after = ctx.fnet(x)
    for k in before:
        assert np.array_equal(before[k], during[k]) and np.array_equal(before[k], after[k]), k
    assert np.array_equal(ctx.fnet_layers(x[:5]), acts)


def test_reload_invalidates_the_calibrator(ctx, shipped):
    from edison_amd import _lib
    m, x, per = shipped
    ctx.fnet_load(FIXTURE)
    cal = ctx.calibrator()
    cal.add(x[:3])
    ctx.fnet_load(FIXTURE)                                  # the same bytes: still another load
    for call in (lambda: cal.add(x[:3]), cal.result, cal.info):
        with pytest.raises(_lib.EdisonError) as e:
            call()
        assert e.value.code == _lib.E_NO_MODEL and "another float network was loaded" in str(e.value)
    cal.close()
    with ctx.calibrator() as fresh:
        fresh.add(x[:3])
        _same(fresh.result(), _merged(per, 0, 3), "a new calibrator")


# ---- sweep networks ---------------------------------------------------------------------------------------------------------------
def _patch_bias_padding(blob, value):
    """Every conv record's bias padding (channels out_c .. n_pad - 1 of the blob) set to `value`."""
    b = bytearray(blob)
    nl, kwb = struct.unpack_from("<i", b, 8)[0], struct.unpack_from("<i", b, 28)[0]
    off = 32 + 64 * nl + kwb
    for i in range(nl):
        v = struct.unpack_from("<16i", b, 32 + 64 * i)
        if v[0] != cube_import.T_CONV:
            continue
        off += 4 * v[14] * v[15]
        for c in range(v[6], v[15]):
            struct.pack_into("<f", b, off + 4 * c, value)
        off += 4 * v[15]
    assert off == len(b)
    return bytes(b)


def _sweep_case(name):
    if name == "batch1":
        rng = np.random.default_rng(41)
        L = dict(type=cube_import.T_CONV, inp=(8, 280, 1), out=(1, 1, 16), k=(8, 280), s=(1, 1), p=(1, 1), relu=0,
                 w=(rng.normal(0, 1, (16, 8, 280, 1)) / 47.0).astype(np.float32), b=rng.normal(0, 0.1, 16).astype(np.float32))
        m = dict(in_shape=(8, 280, 1), layers=[L, dict(type=cube_import.T_SOFTMAX, inp=(1, 1, 16), out=(1, 1, 16))])
        return cube_import.build_blob(m), "pool41_tail", 1
    row = dict(pad_rows_big_bias="pool41_tail", pad_channels="pool22_trunc_hw", neg_bias_relu="pool21_trunc_h", trunc_pool_no_relu="pool12_trunc_w")[name]
    m = fr.model(row)
    first = fh.conv_records(m)[0]
    if name == "pad_rows_big_bias":
        first["b"] = (first["b"] + 40.0).astype(np.float32)
    if name == "neg_bias_relu":
        assert first["relu"] == 1
        first["b"] = np.full_like(first["b"], -30.0)
    if name == "trunc_pool_no_relu":
        assert first["relu"] == 0 and first["p"] == (1, 2)
    blob = cube_import.build_blob(m)
    if name == "pad_channels":
        assert [L["out"][2] for L in fh.conv_records(m)] == [17, 4]
        blob = _patch_bias_padding(blob, 1.0e6)
    return blob, row, 16


@pytest.mark.parametrize("name", ["pad_rows_big_bias", "pad_channels", "neg_bias_relu", "trunc_pool_no_relu", "batch1"])
def test_sweep_network_stats_bit_equal(ctx, name):
    blob, row, batch = _sweep_case(name)
    m = cube_import.read_blob(blob)
    ctx.fnet_load(blob)
    in_n = int(np.prod(m["in_shape"]))
    n = 3 * batch + 2
    x = fr.inputs(row, n, in_n) if name != "batch1" else np.random.default_rng(4).normal(0, 1, (n, in_n)).astype(np.float32)
    if name == "neg_bias_relu":
        x = np.clip(x, -3, 3)                                # |acc| stays below the bias: every output is negative before ReLU
    with ctx.calibrator() as cal:
        assert cal.batch == batch
        for k in sorted({1, batch + 1, n}):
            cal.reset()
            cal.add(x[:k])
            got, want = cal.result(), fh.stats(m, x[:k])
            _same(got, want, "%s, n = %d" % (name, k))
            assert (got["hist"].sum(axis=1) == got["count"]).all()
    if name == "neg_bias_relu":
        assert not fh.run(m, x)[0].any() and want["absmax"][1] > np.float32(20).view(np.uint32)
    if name == "pad_channels":
        assert (want["absmax"][1:].view(np.float32) < 1.0e5).all()
    if name == "trunc_pool_no_relu":
        assert want["count"][1] == n * 4 * 8 * 5              # 4 x 9 conv outputs: 8 columns feed the pool, the ninth is dropped


def test_a_network_that_fills_the_lds_is_refused(ctx):
    from edison_amd import _lib
    ctx.fnet_load(fr.blob("batch1_lds_max"))
    assert ctx.fnet_info()["lds_bytes"] + 4 * 257 > 160 * 1024
    with pytest.raises(_lib.EdisonError) as e:
        ctx.calibrator()
    assert e.value.code == fpl.E_NO_IMPL and "histogram" in str(e.value)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_fixture_rows_end_to_end(ctx, golden):
    """GPU statistic -> blob: byte-equal to the blob of the host statistic; the int8 kernel on it equals net_ref; its argmax is the
    float network's."""
    m, x = fh.load(FIXTURE), _fixture_rows(golden)
    ctx.fnet_load(FIXTURE)
    with ctx.calibrator() as cal:
        cal.add(x)
        stats = cal.result()
    blob, rep = qz.quantize(m, stats)
    want_blob, want_rep = qz.quantize(m, fh.stats(m, x))
    assert blob == want_blob and rep["input"]["dec"] == -3
    xi = qz.quantize_input(x, rep["input"]["dec"])
    ctx.load_model_bytes(blob)
    got, ref = ctx.net(xi), net_ref.run(blob, xi)
    assert np.array_equal(got["logits"], ref["logits"]) and np.array_equal(got["softmax"], ref["softmax"])
    assert np.array_equal(got["argmax"], ref["argmax"])
    assert got["argmax"].tolist() == ctx.fnet(x)["argmax"].tolist() == [0, 7, 9, 8, 8]


def test_context_quantize_audio_to_class(ctx, golden):
    """Context.quantize on the five fixture utterances, then kws_geom at the reported net_input_scale: the "edison" utterance is
    class 0 with the int8 graph."""
    from edison_amd.kws.geometry import KwsGeometry
    names = [str(n) for n in golden["names"]]
    audio = np.stack([golden["audio_" + n] for n in names])
    ctx.fnet_load(FIXTURE)
    blob, rep = ctx.quantize(audio, chunk=2, return_features=True)
    assert np.array_equal(rep["features"], ctx.kws_float(audio.ravel())["feat"])
    assert rep["float_argmax"].tolist() == [0, 7, 9, 8, 8]
    want_blob, _ = qz.quantize(fh.load(FIXTURE), fh.stats(fh.load(FIXTURE), rep["features"]))
    assert blob == want_blob
    assert rep["net_input_scale"] == 0.125
    ctx.load_model_bytes(blob)
    g = KwsGeometry.from_config(net_input_scale=rep["net_input_scale"])
    r = ctx.kws_geom(golden["audio_edison"], g)
    assert r["argmax"].tolist() == [0]


def test_command_line(ctx, golden, tmp_path):
    """kws quantize: the blob and the header it writes are quantize()'s, the report and the agreement are printed."""
    import io
    from edison_amd import nnom_import
    from edison_amd.kws import kws_quantize
    names = [str(n) for n in golden["names"]]
    np.save(tmp_path / "audio.npy", np.stack([golden["audio_" + n] for n in names]))
    out = io.StringIO()
    blob, rep = kws_quantize.run(FIXTURE, str(tmp_path / "audio.npy"), str(tmp_path / "q.ednn"), weights_h=str(tmp_path / "weights.h"), ctx=ctx, out=out)
    assert (tmp_path / "q.ednn").read_bytes() == blob and rep["agreement"] == 1.0
    shape, layers = nnom_import.parse_weights_h((tmp_path / "weights.h").read_text())
    assert nnom_import.build_blob(shape, layers) == blob
    text = out.getvalue()
    assert "conv2d_1" in text and "net_input_scale 0.125" in text and "5 of 5 calibration utterances" in text
    _, rep_s = kws_quantize.run(FIXTURE, str(tmp_path / "audio.npy"), str(tmp_path / "s.ednn"), saturate=0.01, ctx=ctx, out=io.StringIO())
    assert rep_s["method"] == "saturate" and rep_s["input"]["dec"] >= rep["input"]["dec"]
