"""CPU tests of the any-geometry stream's plumbing (no GPU): the C-ABI declares and the binding exposes edison_stream_geom_*, and the
reference answer the GPU tests build frame by frame (stream_drive.oracle_rows) agrees with the batch form of the host flow wherever a
window is full."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["default_opts", "create", "destroy", "reset", "push", "push_dev", "push_n_dev", "frames_seen", "filtered", "filtered_dev", "fsm",
         "fsm_dev"]


def test_header_and_binding_declare_the_stream():
    from edison_amd import _lib
    text = open(os.path.join(ROOT, "include", "edison_hip.h")).read()
    declared = set(re.findall(r"\b(edison_stream_geom_\w+)\s*\(", text))
    assert declared == {"edison_stream_geom_" + n for n in NAMES}
    assert declared <= set(_lib.SIGNATURES)
    assert [f for f, _ in _lib.StreamGeomOpts._fields_] == ["chunk_frames", "filter", "fsm", "filter_alpha", "true_threshold"]


def test_the_stream_is_built():
    from edison_amd import build
    for name in ("edison_stream_bank.hip", "edison_stream_core.hip"):
        assert name in build.HIP_SOURCES
        assert os.path.exists(os.path.join(build.CSRC, name))
    assert "edison_stream_core.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "edison_stream_core.h"))


@pytest.mark.parametrize("name", ["shipped", "square", "kws_small", "odd_no_softmax"])
def test_frame_by_frame_rows_equal_the_batch_host_flow(oracle_mod, name):
    """The GPU tests' reference: rows of the zero-led recording, windowed oldest first. For k >= F - 1 window k equals the batch host
    flow's features of the utterance at (k - F + 1) * frame_step -- also where frame_step > frame_len (kws_small)."""
    import geom_sweep
    from geom_sweep import GEOMS, geom
    from stream_drive import oracle_rows, recording, tail
    g = geom() if name == "shipped" else geom(**GEOMS[name])
    F = g.frame_count
    K = F + 6
    x = recording(g, K, 3)
    rows = oracle_rows(oracle_mod, g, x)
    r = np.concatenate([np.zeros((F - 1, g.num_mfcc), np.int8), rows])
    z = np.concatenate([np.zeros(tail(g), np.int16), x])
    starts = [(k - F + 1) * g.frame_step for k in range(F - 1, K)]
    want = geom_sweep.oracle_feat(oracle_mod, geom_sweep.oracle_mfcc(oracle_mod, z, g, starts), g)
    got = np.stack([r[k:k + F].reshape(-1) for k in range(F - 1, K)])   # rows k - F + 1 .. k
    assert np.array_equal(got, want)
    # the first F - 1 windows start with zero rows: window 0 is F - 1 zero rows and frame 0's row
    assert not r[:F - 1].any() and np.array_equal(r[F - 1], rows[0])
