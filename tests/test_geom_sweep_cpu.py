"""CPU tests of the geometry sweep (tests/geom_sweep.py) that tests/test_gpu_geom_sweep.py runs: the table reaches every code path of
ed_mfcc_geom_kernel as the host plans it, its rows fit a graph input, the restated plan gives DESIGN.md section 11's numbers, and the
oracle the GPU rows are compared with is itself right at the tiny lengths outside its pinned range, and every row's data is sensitive
enough to test something."""
import math

import numpy as np
import pytest

import geom_sweep as gs


def test_the_rows_cover_every_path():
    """team 64 / 256 x {packed Stockham, odd Stockham, direct DFT}, and radices 2, 3, 4, 5 in both teams; each row's note names the
    path the restated plan gives it."""
    want = {(t, k) for t in (64, 256) for k in ("packed", "odd", "direct")} | {(t, "radix %d" % r) for t in (64, 256) for r in (2, 3, 4, 5)}
    seen = set()
    for name, (kw, note) in gs.ROWS.items():
        p = gs.row_plan(name)
        seen.add((p["team"], p["kind"]))
        seen |= {(p["team"], "radix %d" % r) for r in p["radices"]}
        assert note.startswith("wave" if p["team"] == 64 else "workgroup"), (name, note, p["team"])
        if p["kind"] == "direct":
            assert "direct DFT" in note, (name, note)
        else:
            assert "%s M=%d" % (p["kind"], p["M"]) in note, (name, note, p)
            assert int(np.prod(p["radices"])) == p["M"]
    missing = sorted(want - seen)
    assert not missing, "paths no row takes: %s" % missing


def test_rows_fit_a_graph_and_the_frame_arithmetic():
    for name in gs.ROWS:
        g = gs.geometry(name)
        assert 4 <= g.frame_len <= 4096 and 1 <= g.mel_nbins <= 256, name
        assert g.first_mfcc + g.num_mfcc <= g.mel_nbins, name
        assert 1 <= g.frame_count and g.n_features <= gs.MAX_NET_IN, (name, g.n_features)
        assert (g.frame_count - 1) * g.frame_step + g.frame_len <= g.n_samples, name
        n = gs.n_utterances(g, gs.min_frames(name))
        assert n * g.frame_count >= gs.min_frames(name) and n >= 5, (name, n)   # every class of the signal mix appears
    g = gs.geometry("count_lt_fit")
    assert g.frame_count == 50 < 1 + (g.n_samples - g.frame_len) // g.frame_step
    assert gs.geometry("gaps").frame_step > gs.geometry("gaps").frame_len and gs.geometry("step1").frame_step == 1
    assert gs.geometry("above_nyquist").upper_edge_hertz > gs.geometry("above_nyquist").sample_rate / 2


@pytest.mark.parametrize("N, nm, team, slice_bytes, kind", [
    (1024, 32, 64, 16640, "packed"),    # 16.3 KiB per wave
    (512, 20, 64, 8352, "packed"),      # 8.2 KiB per wave
    (441, 16, 64, 5440, "direct"),      # 5.3 KiB per wave
    (1200, 40, 64, 19520, "packed"),    # the team boundary at one N: 19.1 KiB ...
    (1200, 256, 256, 21248, "packed"),  # ... and 20.75 KiB
    (3645, 128, 256, 117664, "odd"),    # 115 KiB: one workgroup per CU
])
def test_restated_plan_gives_the_design_numbers(N, nm, team, slice_bytes, kind):
    p = gs.plan(N, nm)
    assert (p["team"], p["slice_bytes"], p["kind"]) == (team, slice_bytes, kind)
    assert gs.plan(4, 1)["radices"] == [2] and gs.plan(5, 1)["radices"] == [5] and gs.plan(7, 1)["kind"] == "direct"
    assert gs.plan(4094, 1)["kind"] == "direct" and gs.plan(4093, 1)["kind"] == "direct" and gs.plan(4096, 1)["radices"] == [4] * 5 + [2]


@pytest.mark.parametrize("name", sorted(gs.ROWS))
def test_row_is_sensitive(oracle_mod, name):
    """The guard of every row tests/test_gpu_geom_sweep.py runs: its scale puts the 99th percentile of |y scale| in (63.5, 127] (no
    power of two does better), at least half of its oracle features are neither 0 nor clipped, and at least half of its frames
    differ from its most common feature vector -- otherwise the row would not test anything."""
    g, audio, y, feat = gs.row_data(name)
    assert audio.shape[0] * g.frame_count >= gs.min_frames(name)
    p = float(np.percentile(np.abs(y), 99)) * g.net_input_scale
    assert 63.5 < p <= 127.0, p
    assert gs.live_fraction(feat) >= 0.5, gs.live_fraction(feat)
    assert gs.varying_fraction(feat, g.num_mfcc) >= 0.5, gs.varying_fraction(feat, g.num_mfcc)


def test_sensitive_scale():
    y = np.linspace(-3.0, 3.0, 1001)
    s = gs.sensitive_scale(y)
    p = np.percentile(np.abs(y), 99) * s
    assert s == 32.0 and 63.5 < p <= 127.0
    assert gs.live_fraction(np.array([0, 1, -128, 127, 5], np.int8)) == 0.4


def _naive_mfcc(x, variant, N, step, nm, fs, lo, hi, scale, use_log):
    """MFCC A / B written out from the definitions: a DFT summed term by term, triangular mel filters on the HTK mel scale between
    lo and hi over the linear bins 0 .. fs/2 (the DC row zero), scipy's unnormalised DCT-II, the variant's constants."""
    x = np.asarray(x, np.float64)
    nb = N // 2 if variant == "A" else N // 2 + 1
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    edges = [mel(lo) + (mel(hi) - mel(lo)) * i / (nm + 1) for i in range(nm + 2)]
    W = np.zeros((nb, nm))
    for k in range(1, nb):
        m = mel(k * (fs / 2) / (nb - 1))
        for j in range(nm):
            W[k, j] = max(0.0, min((m - edges[j]) / (edges[j + 1] - edges[j]), (edges[j + 2] - m) / (edges[j + 2] - edges[j + 1])))
    n_frames = 1 + (len(x) - N) // step
    out = np.zeros((n_frames, nm))
    for f in range(n_frames):
        fr = x[f * step:f * step + N]
        s = np.zeros(nb)
        for k in range(nb):
            re = sum(fr[n] * math.cos(2 * math.pi * k * n / N) for n in range(N))
            im = -sum(fr[n] * math.sin(2 * math.pi * k * n / N) for n in range(N))
            s[k] = math.hypot(re, im) if variant == "A" else math.hypot(re / 1024, im / 1024) / math.sqrt(2)
        e = s @ W if variant == "A" else (s @ (scale * W)) / scale
        l = np.log(e + 1e-6) if variant == "A" or use_log else e
        for c in range(nm):
            y = 2 * sum(l[n] * math.cos(math.pi * c * (2 * n + 1) / (2 * nm)) for n in range(nm))
            out[f, c] = y / (math.sqrt(2 * nm) if variant == "A" else 64.0)
    return out


@pytest.mark.parametrize("variant, N, nm, use_log", [("B", 4, 1, False), ("A", 4, 1, True), ("A", 5, 4, True), ("B", 5, 3, True),
                                                      ("B", 7, 4, False), ("A", 7, 1, True), ("B", 8, 256, True)])
def test_oracle_at_tiny_lengths_equals_a_naive_dft(oracle_mod, variant, N, nm, use_log):
    """oracle.mfcc_numpy at N = 4, 5, 7, 8 and mel_nbins 1 / 256 (outside the lengths test_oracle.py pins on the reference) equals
    the definitions written out."""
    rng = np.random.default_rng(N * 1000 + nm)
    x = np.clip(rng.normal(0, 3000, 40 * N), -32768, 32767).astype(np.int16)
    for fs, lo, hi in ((16000.0, 80.0, 7600.0), (8000.0, 0.0, 5000.0)):
        want = _naive_mfcc(x, variant, N, N, nm, fs, lo, hi, 128.0, use_log)
        got = oracle_mod.mfcc_numpy(x, oracle_mod.VARIANT_A if variant == "A" else oracle_mod.VARIANT_B, N, N, num_mel_bins=nm, sample_rate=fs,
                                    lower_edge_hertz=lo, upper_edge_hertz=hi, mel_mtx_scale=128.0, use_log=use_log)
        assert got.shape == want.shape
        tol = 1e-11 * max(1.0, float(np.abs(want).max()))
        assert np.abs(got - want).max() <= tol, (fs, np.abs(got - want).max())
