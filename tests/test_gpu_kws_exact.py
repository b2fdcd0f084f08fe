"""GPU tests of the exact KWS mode (edison_kws_set_exact / Context.kws_exact): with it on, the int8 features, logits, softmax and
argmax of a variant-B KWS call equal the float64 host flow's (oracle.mfcc -> oracle.net_input -> oracle.cnn) bit for bit, where
the default fp32 path is allowed to land one int8 step off."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UL = 31 * 1024
N_THREADS = max(1, min(32, os.cpu_count() or 1))
# flagged fraction of the bench mix (tools/fuzz_kws_exact.py measures it per class)
BENCH_MIX_FLAG_CEILING = 0.08


def _fill(out, kind, rng):
    """out: int16 [n, L] filled with one signal class."""
    n, L = out.shape
    t = np.arange(L, dtype=np.float64) / 16000.0
    for lo in range(0, n, 512):
        m = min(512, n - lo)
        if kind == "bench":           # bench.py's mix: speech-level noise + the two tones
            ph = rng.random((m, 2)) * 2 * np.pi
            x = rng.normal(0, 3000, (m, L)) + 1000.0 * np.cos(2 * np.pi * 1000.0 * t + ph[:, :1]) + 500.0 * np.cos(2 * np.pi * 125.0 * t + ph[:, 1:])
        elif kind == "speech":        # test_kws_batch_vs_oracle's first part
            x = rng.normal(0, 3000, (m, L))
        elif kind == "quiet":         # 1 % of full scale
            x = rng.normal(0, 0.01 * 32767, (m, L))
        elif kind == "silence":
            x = np.zeros((m, L))
        elif kind == "dc":            # large DC offset + quiet noise
            x = rng.uniform(-30000, 30000, (m, 1)) + rng.normal(0, 30, (m, L))
        elif kind == "oob_tone":      # full-scale 7.95 kHz tone, above the 80..7600 Hz mel band, + quiet noise
            ph = rng.random((m, 1)) * 2 * np.pi
            x = 32000.0 * np.cos(2 * np.pi * 7950.0 * t + ph) + rng.normal(0, 30, (m, L))
        elif kind == "square":        # full-scale square waves of random period and phase
            per = rng.integers(4, 400, (m, 1))
            ph = rng.integers(0, 400, (m, 1))
            x = np.where(((np.arange(L)[None, :] + ph) // per) % 2 == 0, 32767.0, -32768.0)
        elif kind == "impulse":       # one full-scale sample per frame at a random place
            x = np.zeros((m, L))
            pos = rng.integers(0, 1024, (m, 31)) + 1024 * np.arange(31)[None, :]
            np.put_along_axis(x, pos, rng.choice([-32768.0, 32767.0], (m, 31)), axis=1)
        else:
            raise ValueError(kind)
        out[lo:lo + m] = np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _audio(kinds, n_each, seed, stride=UL):
    rng = np.random.default_rng(seed)
    a = np.zeros((len(kinds) * n_each, stride), np.int16)
    for i, k in enumerate(kinds):
        _fill(a[i * n_each:(i + 1) * n_each, :UL], k, rng)
    return a


def _ref_feat(oracle_mod, a):
    """oracle.net_input(oracle.mfcc(u, B)[:, :13]) of every utterance (rows of a, first 31*1024 samples), [n, 403]."""
    n = a.shape[0]
    out = np.zeros((n, 403), np.int8)
    for lo in range(0, n, 2048):
        x = np.ascontiguousarray(a[lo:lo + 2048, :UL]).reshape(-1)
        m = oracle_mod.mfcc(x, 1, n_frames=x.size // 1024, n_threads=N_THREADS)
        out[lo:lo + 2048] = oracle_mod.net_input(m[:, :13]).reshape(-1, 403)
    return out


def _kws(ctx, a, exact):
    return ctx.kws(a.reshape(-1), n_utt=a.shape[0], utt_stride=a.shape[1], exact=exact)


def _kws_t(ctx, a, exact):
    import torch
    dev = torch.device("cuda", 0)
    n = a.shape[0]
    audio = torch.from_numpy(a.reshape(-1)).to(dev)
    feat = torch.full((n, 403), 99, dtype=torch.int8, device=dev)
    lo, so = torch.zeros((n, 10), dtype=torch.int8, device=dev), torch.zeros((n, 10), dtype=torch.int8, device=dev)
    am = torch.zeros((n,), dtype=torch.int32, device=dev)
    ctx.use_torch_stream()
    try:
        ctx.kws_t(audio, n, a.shape[1], feat=feat, logits=lo, softmax=so, argmax=am, exact=exact)
        torch.cuda.synchronize()
    finally:
        ctx.use_own_stream()
    return dict(feat=feat.cpu().numpy(), logits=lo.cpu().numpy(), softmax=so.cpu().numpy(), argmax=am.cpu().numpy())


def _assert_oracle(r, ref_feat, ref_cnn, what):
    bad = np.flatnonzero((r["feat"] != ref_feat).any(axis=1))
    assert bad.size == 0, (what, "utterances with features != oracle", bad[:10], bad.size)
    for k in ("logits", "softmax", "argmax"):
        assert np.array_equal(r[k], ref_cnn[k]), (what, k)


def test_exact_end_to_end_16k_utterances(ctx, oracle_mod, oracle_model):
    """test_kws_batch_vs_oracle's mix at 16 384 utterances: features, logits, softmax, argmax equal the host flow's, host and _dev."""
    n3 = 16384 // 4
    a = _audio(["speech", "quiet", "silence", "speech"], n3, 2101, stride=32000)
    rng = np.random.default_rng(5)
    a[:, UL:] = rng.integers(-3000, 3000, (a.shape[0], 32000 - UL), dtype=np.int16)  # samples the utterances do not use
    ref = _ref_feat(oracle_mod, a)
    ref_cnn = oracle_mod.cnn(oracle_model, ref, n_threads=N_THREADS)
    _assert_oracle(_kws(ctx, a, True), ref, ref_cnn, "host, stride 32000")
    _assert_oracle(_kws_t(ctx, a, True), ref, ref_cnn, "dev, stride 32000")
    b = np.ascontiguousarray(a[:, :UL])
    _assert_oracle(_kws_t(ctx, b, True), ref, ref_cnn, "dev, stride 31744")


def test_exact_fixes_the_default_paths_flips(ctx, oracle_mod, oracle_model):
    """>= 262 144 frames where the fp32 default path lands a feature one step off somewhere; exact mode matches the oracle on
    those utterances and on the whole sample."""
    n_each = 8464 // 4
    a = _audio(["bench", "bench", "oob_tone", "square"], n_each, 2202)
    assert a.shape[0] * 31 >= 262144
    ref = _ref_feat(oracle_mod, a)
    default = _kws(ctx, a, False)
    diff = np.flatnonzero((default["feat"] != ref).any(axis=1))
    assert diff.size >= 1, "the default path agreed with the oracle everywhere: enlarge the sample"
    assert np.abs(default["feat"].astype(int) - ref.astype(int)).max() == 1
    ex = _kws(ctx, a, True)
    assert np.array_equal(ex["feat"][diff], ref[diff])
    ref_cnn = oracle_mod.cnn(oracle_model, ref, n_threads=N_THREADS)
    _assert_oracle(ex, ref, ref_cnn, "whole sample")


@pytest.mark.parametrize("kind", ["dc", "oob_tone", "square", "impulse", "silence"])
def test_exact_adversarial_classes(ctx, oracle_mod, oracle_model, kind):
    a = _audio([kind], 1024, 2303 + len(kind))
    ref = _ref_feat(oracle_mod, a)
    ref_cnn = oracle_mod.cnn(oracle_model, ref, n_threads=N_THREADS)
    _assert_oracle(_kws(ctx, a, True), ref, ref_cnn, kind)


def test_exact_stats(ctx):
    a = _audio(["silence"], 256, 2404)
    _kws(ctx, a, True)
    assert ctx.kws_exact_stats() == (0, 31 * 256)
    n = 2048
    b = _audio(["bench"], n, 2405)
    _kws(ctx, b, True)
    flagged, total = ctx.kws_exact_stats()
    assert total == 31 * n
    assert 0 < flagged < BENCH_MIX_FLAG_CEILING * total, (flagged, total)


def test_exact_off_means_unchanged(ctx):
    a = _audio(["bench", "quiet", "oob_tone"], 256, 2506)
    assert not ctx.kws_exact
    before = _kws(ctx, a, None)
    before_t = _kws_t(ctx, a, None)
    ctx.kws_exact = True
    try:
        assert ctx.kws_exact
        _kws(ctx, a, None)
    finally:
        ctx.kws_exact = False
    assert not ctx.kws_exact
    after = _kws(ctx, a, None)
    after_t = _kws_t(ctx, a, None)
    for k in ("feat", "logits", "softmax", "argmax"):
        assert np.array_equal(before[k], after[k]), k
        assert np.array_equal(before_t[k], after_t[k]), k
        assert np.array_equal(before[k], before_t[k]), k


def test_exact_per_call_argument_restores_the_mode(ctx):
    a = _audio(["bench"], 64, 2607)
    ctx.kws_exact = False
    _kws(ctx, a, True)
    assert not ctx.kws_exact
    ctx.kws_exact = True
    try:
        _kws(ctx, a, False)
        assert ctx.kws_exact
    finally:
        ctx.kws_exact = False


def test_exact_mode_from_the_environment():
    env = dict(os.environ, EDISON_KWS_EXACT="1")
    code = "from edison_amd.context import Context; c = Context(0); print('exact', int(c.kws_exact)); c.close()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "exact 1" in r.stdout


def test_exact_sharded_equals_unsharded(ctx, oracle_mod, oracle_model):
    """edison_kws_batch_sharded_dev / _total_dev in exact mode, outside a communicator and in a world of one through RCCL."""
    import torch
    from edison_amd import parallel
    from edison_amd.context import Context
    a = _audio(["bench", "oob_tone"], 200, 2708)
    n = a.shape[0]
    ref = _ref_feat(oracle_mod, a)
    ref_cnn = oracle_mod.cnn(oracle_model, ref, n_threads=N_THREADS)
    c = Context(0)
    try:
        dev = torch.device("cuda", 0)
        c.use_torch_stream()
        audio = torch.from_numpy(a.reshape(-1)).to(dev)
        feat = torch.zeros((n, 403), dtype=torch.int8, device=dev)
        lo, so = torch.zeros((n, 10), dtype=torch.int8, device=dev), torch.zeros((n, 10), dtype=torch.int8, device=dev)
        am = torch.zeros((n,), dtype=torch.int32, device=dev)

        def check(all_logits, what):
            torch.cuda.synchronize()
            r = dict(feat=feat.cpu().numpy(), logits=lo.cpu().numpy(), softmax=so.cpu().numpy(), argmax=am.cpu().numpy())
            _assert_oracle(r, ref, ref_cnn, what)
            assert np.array_equal(all_logits.cpu().numpy(), ref_cnn["logits"]), what

        all0 = torch.full((n, 10), 99, dtype=torch.int8, device=dev)
        c.kws_sharded_t(audio, n, UL, all0, feat=feat, logits=lo, softmax=so, argmax=am, exact=True)
        check(all0, "sharded, no communicator")
        c.dist_init(parallel.dist_unique_id(), 0, 1)
        all1 = torch.full((n, 10), 77, dtype=torch.int8, device=dev)
        c.kws_sharded_t(audio, n, UL, all1, feat=feat, logits=lo, softmax=so, argmax=am, exact=True)
        check(all1, "sharded, world of one")
        all2 = torch.full((n, 10), 66, dtype=torch.int8, device=dev)
        c.kws_sharded_total_t(audio, n, UL, all2, feat=feat, logits=lo, softmax=so, argmax=am, exact=True)
        check(all2, "sharded total, world of one")
        assert not c.kws_exact
        c.dist_shutdown()
    finally:
        c.close()
