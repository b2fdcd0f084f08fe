"""The geometry sweep: named MFCC geometries (kws.geometry.KwsGeometry fields) chosen so that together they take every code path of
the any-geometry kernels -- ed_mfcc_geom_kernel (csrc/mfcc_geom_kernels.hip, behind edison_kws_geom_batch*) and
ed_mfcc_generic_kernel (csrc/mfcc_generic_kernels.hip, behind edison_mfcc_generic*) -- over the whole range they accept:
frame_len 4 .. 4096, mel_nbins 1 .. 256, any sample rate and edges, variants A and B with or without log, any first_mfcc / num_mfcc.

Test infrastructure, not a test: tests/test_geom_sweep_cpu.py checks that the table covers every path of the restated plan,
tests/test_gpu_geom_sweep.py runs every row against the float64 oracle, tools/fuzz_kws_geom.py --sweep fuzzes them.

`plan` restates the host's choice in geom_tables() (csrc/edison_kws_geom.hip): the radices (plan_radices), packed / odd / direct,
the three LDS regions r0 / r1 / r2 of a team's slice (in doubles) and the team (a wavefront while the slice is at most 20 KiB, the
256-thread workgroup beyond). The note of each row names the path that plan gives it; the CPU test checks the notes against it.

Every row keeps frame_count x num_mfcc <= 32 640, the largest graph input (ED_NET_MAX_LDS / 2).

Also what the geometry tests and tools share besides the rows: GEOMS (the committed alt_models graphs' geometries), geom, header and the
signal mix `signals`."""
import functools
import os

import numpy as np

WAVE_TEAM_BYTES = 20480   # EDG_WAVE_TEAM_BYTES (edison_kws_geom.hip)
MAX_NET_IN = 32640        # ED_NET_MAX_LDS / 2 (edison_internal.h)

# name -> (KwsGeometry fields with variant "A" / "B", the path `plan` takes: team, transform, radices, slice)
ROWS = {
    # the smallest transforms
    "n4_b_mel1": (dict(variant="B", frame_len=4, frame_step=4, n_samples=800, mel_nbins=1, num_mfcc=1),
                  "wave, packed M=2 (one radix-2 stage; the split bin k = M reads Z[0] twice), one mel band"),
    "n5_a": (dict(variant="A", frame_len=5, frame_step=5, n_samples=1000, mel_nbins=4, first_mfcc=1, num_mfcc=3, upper_edge_hertz=12000.0),
             "wave, odd M=5 (radix 5), 2 spectrum bins under 4 mel bands (the upper edge above Nyquist: below it bin 1 meets no band)"),
    "n6_blog_first1": (dict(variant="B", use_log=True, frame_len=6, frame_step=3, n_samples=600, mel_nbins=3, first_mfcc=1, num_mfcc=2),
                       "wave, packed M=3 (radix 3), DCT rows 1 .. 2 (to the last)"),
    "n7_direct": (dict(variant="B", frame_len=7, frame_step=7, n_samples=1400, mel_nbins=4, num_mfcc=4),
                  "wave, direct DFT at odd N"),
    "n8_blog_mel256": (dict(variant="B", use_log=True, frame_len=8, frame_step=8, n_samples=1600, mel_nbins=256, first_mfcc=250, num_mfcc=6),
                       "wave, packed M=4 (radix 4), 5 bins under 256 bands: mostly empty band runs, DCT rows from the end"),
    # odd N on the unpacked load, radices 3 and 5 on a wavefront
    "n15_a": (dict(variant="A", frame_len=15, frame_step=15, n_samples=3000, mel_nbins=6, first_mfcc=1, num_mfcc=5),
              "wave, odd M=15 (3, 5), variant A at odd N: (N-1)/2 bins"),
    "n30_b": (dict(variant="B", frame_len=30, frame_step=20, n_samples=4000, mel_nbins=10, num_mfcc=10),
              "wave, packed M=15 (3, 5)"),
    "n375": (dict(variant="B", frame_len=375, frame_step=250, n_samples=16000, mel_nbins=24, num_mfcc=13),
             "wave, odd M=375 (3, 5, 5, 5)"),
    "n625_a": (dict(variant="A", frame_len=625, frame_step=400, n_samples=16000, mel_nbins=8, first_mfcc=1, num_mfcc=7),
               "wave, odd M=625 (5, 5, 5, 5), 19.6 KiB slice"),
    # the direct DFT on a wavefront
    "n882_blog": (dict(variant="B", use_log=True, frame_len=882, frame_step=441, n_samples=16000, mel_nbins=40, first_mfcc=1, num_mfcc=12),
                  "wave, direct DFT at even N (M = 441 = 3^2 7^2)"),
    "n1026": (dict(variant="B", frame_len=1026, frame_step=513, n_samples=16000, mel_nbins=20, num_mfcc=13),
              "wave, direct DFT at even N (M = 513 = 3^3 19)"),
    "n1023_a": (dict(variant="A", frame_len=1023, frame_step=1023, n_samples=16000, mel_nbins=32, first_mfcc=1, num_mfcc=13),
                "wave, direct DFT at odd N (3 11 31)"),
    # one transform on both sides of the team boundary
    "n1200_m40": (dict(variant="B", frame_len=1200, frame_step=600, n_samples=16000, mel_nbins=40, num_mfcc=13),
                  "wave, packed M=600 (4, 2, 3, 5, 5), 19.1 KiB slice"),
    "n1200_m256": (dict(variant="B", use_log=True, frame_len=1200, frame_step=600, n_samples=16000, mel_nbins=256, first_mfcc=1, num_mfcc=20),
                   "workgroup, packed M=600 (4, 2, 3, 5, 5): 256 mel bands push the slice over 20 KiB"),
    "n1250_m40_a": (dict(variant="A", frame_len=1250, frame_step=625, n_samples=16000, mel_nbins=40, first_mfcc=1, num_mfcc=20),
                    "wave, packed M=625 (5, 5, 5, 5), 19.8 KiB slice"),
    # the workgroup team
    "n1280": (dict(variant="B", frame_len=1280, frame_step=640, n_samples=16000, mel_nbins=32, num_mfcc=13),
              "workgroup, packed M=640 (4, 4, 4, 2, 5)"),
    "n1536_m64": (dict(variant="B", use_log=True, frame_len=1536, frame_step=768, n_samples=16000, mel_nbins=64, first_mfcc=2, num_mfcc=20),
                  "workgroup, packed M=768 (4, 4, 4, 4, 3)"),
    "n2048_a_44k": (dict(variant="A", frame_len=2048, frame_step=1024, n_samples=44100, mel_nbins=40, first_mfcc=1, num_mfcc=13, sample_rate=44100.0,
                         lower_edge_hertz=20.0, upper_edge_hertz=20000.0),
                    "workgroup, packed M=1024 (4, 4, 4, 4, 4), fs 44.1 kHz"),
    "n2187": (dict(variant="B", frame_len=2187, frame_step=1000, n_samples=32000, mel_nbins=32, num_mfcc=13),
              "workgroup, odd M=2187 (3^7)"),
    "n3375_m256": (dict(variant="B", use_log=True, frame_len=3375, frame_step=2000, n_samples=40000, mel_nbins=256, first_mfcc=200, num_mfcc=56),
                   "workgroup, odd M=3375 (3, 3, 3, 5, 5, 5), DCT rows 200 .. 255"),
    "n3645_m128_a": (dict(variant="A", frame_len=3645, frame_step=3645, n_samples=40000, mel_nbins=128, first_mfcc=1, num_mfcc=20),
                     "workgroup, odd M=3645 (3^6 5), 115 KiB slice: one workgroup per CU"),
    "n4093": (dict(variant="B", frame_len=4093, frame_step=2048, n_samples=40000, mel_nbins=32, num_mfcc=8),
              "workgroup, direct DFT at prime N"),
    "n4094_a": (dict(variant="A", frame_len=4094, frame_step=4094, n_samples=45000, mel_nbins=64, first_mfcc=1, num_mfcc=16),
                "workgroup, direct DFT at even N (M = 2047 = 23 89)"),
    "n4096_m256_48k": (dict(variant="B", use_log=True, frame_len=4096, frame_step=2048, n_samples=43008, mel_nbins=256, num_mfcc=256,
                            sample_rate=48000.0, lower_edge_hertz=50.0, upper_edge_hertz=24000.0),
                       "workgroup, packed M=2048 (4, 4, 4, 4, 4, 2), fs 48 kHz, upper edge at Nyquist, all 256 DCT rows"),
    # sample rates and edges
    "fs8k": (dict(variant="B", frame_len=256, frame_step=128, n_samples=8000, mel_nbins=26, num_mfcc=13, sample_rate=8000.0,
                  lower_edge_hertz=60.0, upper_edge_hertz=4000.0),
             "wave, packed M=128 (4, 4, 4, 2), fs 8 kHz, upper edge at Nyquist"),
    "above_nyquist": (dict(variant="B", use_log=True, frame_len=512, frame_step=256, n_samples=16000, mel_nbins=40, first_mfcc=1, num_mfcc=13,
                           upper_edge_hertz=9000.0),
                      "wave, packed M=256 (4, 4, 4, 4), upper edge above Nyquist: the top bands have no bins"),
    # frame shapes
    "gaps": (dict(variant="B", frame_len=320, frame_step=500, n_samples=16000, mel_nbins=20, num_mfcc=10),
             "wave, packed M=160 (4, 4, 2, 5), frame_step > frame_len"),
    "step1": (dict(variant="B", use_log=True, frame_len=64, frame_step=1, n_samples=263, mel_nbins=16, first_mfcc=1, num_mfcc=8),
              "wave, packed M=32 (4, 4, 2), frame_step 1"),
    "count_lt_fit": (dict(variant="A", frame_len=400, frame_step=160, n_samples=16000, frame_count_=50, mel_nbins=40, first_mfcc=1, num_mfcc=13),
                     "wave, packed M=200 (4, 2, 5, 5), an explicit frame_count below the 98 that fit"),
}


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# committed alt_models graph -> the geometry it is run at (its input is frame_count x num_mfcc features)
GEOMS = {
    "kws_small": dict(variant="B", use_log=True, frame_len=512, frame_step=1024, n_samples=32000, mel_nbins=20, first_mfcc=0, num_mfcc=13),
    "same_stride": dict(variant="B", frame_len=800, frame_step=800, n_samples=16000, mel_nbins=40, first_mfcc=1, num_mfcc=12,
                        lower_edge_hertz=20.0, upper_edge_hertz=4000.0, mel_mtx_scale=64.0),
    "square": dict(variant="A", frame_len=480, frame_step=240, n_samples=15600, mel_nbins=24, first_mfcc=0, num_mfcc=16),
    "even_same": dict(variant="B", frame_len=1000, frame_step=500, n_samples=8500, mel_nbins=32, first_mfcc=0, num_mfcc=20, net_input_scale=0.5),
    "odd_no_softmax": dict(variant="B", frame_len=441, frame_step=441, n_samples=11907, mel_nbins=16, first_mfcc=0, num_mfcc=7),
}


def geom(**kw):
    """A KwsGeometry from audio/config.py's with these fields changed (variant "A" / "B" by name)."""
    from edison_amd import _lib
    from edison_amd.kws.geometry import KwsGeometry
    kw = dict(kw)
    if kw.get("variant") in ("A", "B"):
        kw["variant"] = _lib.MFCC_A if kw["variant"] == "A" else _lib.MFCC_B
    return KwsGeometry.from_config(**kw)


def header(name):
    return os.path.join(GOLDEN, "alt_models", name + ".h")


def signals(n_utt, n_samples, seed):
    """int16 [n_utt][n_samples]: silence, low-level noise, tones, clipping-loud noise and the reference's `edison` utterance (at a random
    place and gain), in turn."""
    rng = np.random.default_rng(seed)
    edison = np.load(os.path.join(GOLDEN, "mfcc_geom_golden.npz"))["in_edison"].astype(np.float64)
    t = np.arange(n_samples) / 16000.0
    out = np.zeros((n_utt, n_samples), np.int16)
    for u in range(n_utt):
        kind = u % 5
        if kind == 0:
            x = np.zeros(n_samples)
        elif kind == 1:
            x = rng.normal(0, rng.uniform(0.5, 30.0), n_samples)
        elif kind == 2:
            f = rng.uniform(50.0, 7900.0, 2)
            x = rng.uniform(100, 20000) * np.cos(2 * np.pi * f[0] * t + rng.random() * 6.3) + rng.uniform(0, 3000) * np.cos(2 * np.pi * f[1] * t)
        elif kind == 3:
            x = rng.normal(0, rng.uniform(20000, 60000), n_samples)
        else:
            x = rng.normal(0, 10.0, n_samples)
            e = edison[:n_samples] * rng.uniform(0.3, 4.0)
            at = int(rng.integers(0, max(1, n_samples - e.shape[0] + 1)))
            x[at:at + e.shape[0]] += e
        out[u] = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    return out


def geometry(name, **changes):
    """The row's KwsGeometry (net_input_scale 1 unless changed)."""
    from edison_amd import _lib
    from edison_amd.kws.geometry import KwsGeometry
    kw = dict(ROWS[name][0])
    kw["variant"] = _lib.MFCC_A if kw["variant"] == "A" else _lib.MFCC_B
    kw.update(changes)
    return KwsGeometry.from_config(**kw)


def plan_radices(M):
    """Radices 4, then 2, 3, 5 whose product is M; [] when M has another prime factor (plan_radices in edison_kws_geom.hip)."""
    out = []
    for r in (4, 2, 3, 5):
        while M % r == 0:
            out.append(r)
            M //= r
    return out if M == 1 else []


def plan(N, mel_nbins, variant="B"):
    """geom_tables()'s plan for a frame length, mel bin count and variant ("A" / "B"): a dict with packed, M (0: direct DFT),
    radices, kind ("packed" / "odd" / "direct"), n_bins, r0 / r1 / r2 (doubles), slice_bytes and team (64 / 256)."""
    nb = N // 2 if variant == "A" else N // 2 + 1
    packed = N % 2 == 0
    M = N // 2 if packed else N
    radices = plan_radices(M)
    if not radices:
        M = 0
    if M:
        r0 = r1 = 2 * M
    else:
        r0, r1 = (N + 1) & ~1, (nb + 1) & ~1
    r2 = (mel_nbins + 1) & ~1
    slice_bytes = 8 * (r0 + r1 + r2)
    return dict(packed=packed, M=M, radices=radices, kind="direct" if not M else ("packed" if packed else "odd"), n_bins=nb, r0=r0, r1=r1,
                r2=r2, slice_bytes=slice_bytes, team=64 if slice_bytes <= WAVE_TEAM_BYTES else 256)


def row_plan(name):
    kw = ROWS[name][0]
    return plan(kw["frame_len"], kw["mel_nbins"], kw["variant"])


def min_frames(name):
    """Frames a GPU test runs at this row: 6 000, 1 000 for frames of 2048 samples and more."""
    return 1000 if ROWS[name][0]["frame_len"] >= 2048 else 6000


def n_utterances(g, frames):
    return -(-frames // g.frame_count)


def oracle_mfcc(oracle, rows, g, starts=None):
    """float64 [n_utt][frame_count][num_mfcc]: oracle.mfcc_numpy's coefficients first_mfcc .. first_mfcc + num_mfcc - 1 of each
    utterance: rows [n_utt][>= span] int16, or a flat int16 stream whose utterances begin at `starts`."""
    ov = oracle.VARIANT_A if g.variant == 0 else oracle.VARIANT_B
    F = g.frame_count
    span = (F - 1) * g.frame_step + g.frame_len
    n = len(starts) if starts is not None else rows.shape[0]
    out = np.zeros((n, F, g.num_mfcc))
    for u in range(n):
        x = rows[starts[u]:starts[u] + span] if starts is not None else rows[u, :span]
        m = oracle.mfcc_numpy(x, ov, g.frame_len, g.frame_step, n_frames=F, num_mel_bins=g.mel_nbins, sample_rate=g.sample_rate,
                              lower_edge_hertz=g.lower_edge_hertz, upper_edge_hertz=g.upper_edge_hertz, mel_mtx_scale=g.mel_mtx_scale,
                              use_log=g.use_log)
        out[u] = m[:, g.first_mfcc:g.first_mfcc + g.num_mfcc]
    return out


def oracle_feat(oracle, y, g):
    """int8 [n_utt][frame_count * num_mfcc]: oracle.net_input of the coefficients y (oracle_mfcc) at g.net_input_scale."""
    n = y.shape[0]
    return oracle.net_input(y.reshape(-1, g.num_mfcc), n_coef=g.num_mfcc, scale=g.net_input_scale).reshape(n, -1)


@functools.lru_cache(maxsize=None)
def row_data(name):
    """(geometry at its sensitive scale, audio [n_utt][n_samples], oracle coefficients [n_utt][F][num_mfcc], oracle int8 features
    [n_utt][F * num_mfcc]) of the row at min_frames frames: what the GPU tests run and the CPU guard checks."""
    from dataclasses import replace
    from oracle import oracle
    oracle.build()
    g = geometry(name)
    audio = row_signals(name, g, min_frames(name))
    y = oracle_mfcc(oracle, audio, g)
    g = replace(g, net_input_scale=sensitive_scale(y))
    return g, audio, y, oracle_feat(oracle, y, g)


def sensitive_scale(y):
    """The power of two s that puts the 99th percentile of |y s| in (63.5, 127]: a power of two converts to float32 exactly on both
    sides, and at that scale a relative error of 1e-5 in y moves many features by an int8 step."""
    p = float(np.percentile(np.abs(y), 99))
    assert p > 0.0, "the row's coefficients are all zero"
    return float(2.0 ** np.floor(np.log2(127.0 / p)))


def live_fraction(feat):
    """Share of int8 features that are neither 0 nor clipped (-128 / 127)."""
    f = np.asarray(feat)
    return float(np.mean((f != 0) & (f != 127) & (f != -128)))


def varying_fraction(feat, num_mfcc):
    """Share of frames whose int8 feature vector differs from the row's most common one: features that do not follow the signal
    (a band layout that leaves the coefficients at float64 rounding noise) give 0."""
    v = np.asarray(feat).reshape(-1, num_mfcc)
    _, counts = np.unique(v, axis=0, return_counts=True)
    return 1.0 - counts.max() / v.shape[0]


def dense_graph(g, seed=0, n_out=4):
    """A graph of one Dense layer over a (frame_count, num_mfcc, 1) input, as an .ednn blob for Context.load_model_bytes."""
    from edison_amd import nnom_import
    rng = np.random.default_rng(seed)
    n_in = g.n_features
    assert n_in <= MAX_NET_IN, n_in
    layer = dict(type=3, out=n_out, w=rng.integers(-9, 10, n_out * n_in).astype(np.int8), b=rng.integers(-20, 21, n_out).astype(np.int8),
                 out_rshift=max(0, int(np.ceil(np.log2(9 * 128 * np.sqrt(n_in)))) - 6), bias_lshift=0, relu=0)
    return nnom_import.build_blob((g.frame_count, g.num_mfcc, 1), [layer])


def row_signals(name, g, frames, seed=0):
    """int16 [n_utt][n_samples]: the `signals` mix (silence, quiet noise, tones, clipping-loud noise, the `edison` utterance in noise,
    in turn), enough utterances for `frames` frames, each utterance brought to an RMS level between 1 500 and 6 000 (silence stays
    silence). The mix spans four decades of level; at one net_input_scale per row the quiet classes would round to int8 zero and test
    nothing."""
    s = 1000 + 7 * seed + sorted(ROWS).index(name)
    x = signals(n_utterances(g, frames), g.n_samples, s).astype(np.float64)
    rms = np.sqrt(np.mean(x * x, axis=1))
    level = 3000.0 * 2.0 ** np.random.default_rng(s).uniform(-1.0, 1.0, x.shape[0])
    gain = np.where(rms > 0, level / np.maximum(rms, 1e-30), 0.0)
    return np.clip(np.rint(x * gain[:, None]), -32768, 32767).astype(np.int16)
