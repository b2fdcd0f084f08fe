"""CPU tests of the NNoM example's loop (tests/nnom_kws_ref.py) and of edison_nnom_predict, nnom_predict's result rule in host C
(csrc/legacy.c, csrc/nnom_predict_core.h): no GPU.

  * edison_nnom_predict equals the numpy restatement bit for bit: seeded random rows at 1, 2, 10 and 35 outputs, ties, all zeros, a
    zero sum beside a non-zero maximum, a negative sum, a lone -128 and a lone 127, and all 256 values of a single output;
  * the ring the firmware unrolls oldest row first is the sliding window over the row sequence with zero rows in front: the identity
    the in-place window read of edison_f32_stream_predict rests on, on either side of a ring wrap;
  * the address arithmetic of the rows form of variant D against a brute-force list.
"""
import ctypes

import numpy as np
import pytest

import nnom_kws_ref as ref


def _predict(L, out):
    o = np.ascontiguousarray(out, dtype=np.int8)
    n, n_out = o.shape
    label, prob = np.full(n, 0xdeadbeef, np.uint32), np.full(n, -7.0, np.float32)
    r = L.edison_nnom_predict(o.ctypes.data_as(ctypes.c_void_p), n, n_out, label.ctypes.data_as(ctypes.c_void_p), prob.ctypes.data_as(ctypes.c_void_p))
    assert r == 0
    return label, prob


def _same(L, out):
    label, prob = _predict(L, out)
    wl, wp = ref.predict_rule(out)
    assert np.array_equal(label, wl), np.argwhere(label != wl)[:3]
    assert np.array_equal(prob.view(np.uint32), wp.view(np.uint32)), np.argwhere(prob.view(np.uint32) != wp.view(np.uint32))[:3]
    return label, prob


@pytest.mark.parametrize("n_out", [1, 2, 10, 35])
def test_predict_equals_the_restatement_on_random_rows(built_lib, n_out):
    rng = np.random.default_rng(500 + n_out)
    out = rng.integers(-128, 128, (4000, n_out)).astype(np.int8)
    out[1000:2000] = np.clip(out[1000:2000], 0, 127)                      # what a softmax gives: nothing negative
    out[2000:2500] //= 16                                                 # small values: sums near zero, many ties
    _same(built_lib, out)


def test_predict_edge_cases(built_lib):
    L = built_lib
    for n_out in (2, 10, 35):
        z = np.zeros((1, n_out), np.int8)
        label, prob = _same(L, z)
        assert label[0] == 0 and prob[0] == 0.0                           # all zeros: prob 0, the first index
        tie = z.copy(); tie[0, 1:] = 5; tie[0, 0] = -3
        label, _ = _same(L, tie)
        assert label[0] == 1                                              # ties: the first maximum wins
        tie[0, 0] = 5
        assert _same(L, tie)[0][0] == 0
        zs = z.copy(); zs[0, 0], zs[0, -1] = -7, 7                        # sum 0 beside a non-zero maximum
        label, prob = _same(L, zs)
        assert label[0] == n_out - 1 and prob[0] == 0.0
        neg = np.full((1, n_out), -20, np.int8); neg[0, n_out // 2] = 9   # a negative sum keeps the C quotient
        label, prob = _same(L, neg)
        assert label[0] == n_out // 2 and prob[0] < 0
        lo = z.copy(); lo[0, n_out - 1] = -128                            # a lone -128: the maximum is a zero
        label, prob = _same(L, lo)
        assert label[0] == 0 and prob[0] == 0.0
        hi = z.copy(); hi[0, n_out - 1] = 127                             # a lone 127
        label, prob = _same(L, hi)
        assert label[0] == n_out - 1 and prob[0] == 1.0
        full = np.full((1, n_out), -128, np.int8)
        _same(L, full)
        _same(L, np.full((1, n_out), 127, np.int8))
    one = np.arange(-128, 128, dtype=np.int16).astype(np.int8).reshape(256, 1)          # a single output: all 256 values
    label, prob = _same(L, one)
    assert label.sum() == 127 - 64 + 1 and label[128 + 64] == 1 and label[128 + 63] == 0   # 64 / 127 >= 0.5 > 63 / 127
    assert L.edison_nnom_predict(None, 0, 10, None, None) == 0
    assert L.edison_nnom_predict(None, 1, 10, None, None) != 0 and L.edison_nnom_predict(one.ctypes.data_as(ctypes.c_void_p), 1, 0, None, None) != 0
    lab = np.zeros(256, np.uint32)                                        # prob may be NULL
    assert L.edison_nnom_predict(one.ctypes.data_as(ctypes.c_void_p), 256, 1, lab.ctypes.data_as(ctypes.c_void_p), None) == 0
    assert np.array_equal(lab, label)


def _toy(n_out):
    """A feature function that tells every frame from every other: a hash of its samples"""
    w = (np.arange(ref.EVENT, dtype=np.int64) * 2654435761 % 251)[:, None] + np.arange(n_out, dtype=np.int64)[None, :] * 17 + 1

    def fn(frame):
        assert frame.shape == (ref.EVENT,)
        return ((frame.astype(np.int64) @ w) % 256 - 128).astype(np.int8)
    return fn


@pytest.mark.parametrize("rows", [2, 3, 12, 63])
def test_ring_unrolled_oldest_first_is_the_sliding_window(rows):
    n_out = 5
    fn = _toy(n_out)
    wrap = -(-rows // 2)                                                  # the first event whose second row wraps the ring
    rng = np.random.default_rng(rows)
    for n_ev in sorted({1, max(wrap - 1, 1), wrap, wrap + 1, 2 * wrap + 3, rows + 2}):
        x = rng.integers(-3000, 3000, n_ev * ref.EVENT).astype(np.int16)
        ring = ref.ring_loop(fn, x, rows, n_out)
        seq = ref.row_sequence(fn, x, n_out)
        assert seq.shape == (2 * n_ev, n_out) and len({r.tobytes() for r in seq}) == 2 * n_ev, "the toy rows must all differ"
        slide = ref.sliding_windows(seq, rows)
        assert ring.shape == slide.shape == (n_ev, rows, n_out)
        assert np.array_equal(ring, slide), (rows, n_ev, np.argwhere(ring != slide)[0])
        # the newest two rows of window e are the event's two frames; zero rows stand in front until the ring is full
        for e in range(n_ev):
            assert np.array_equal(slide[e, -2:], seq[2 * e:2 * e + 2]) if rows >= 2 else True
            assert not slide[e, :max(rows - 2 * e - 2, 0)].any()


@pytest.mark.parametrize("frames_per_row", [1, 2, 3, 12, 13])
def test_rows_form_addresses(frames_per_row):
    frame_len = 512
    for n_rows, row_stride, frame_step in ((1, 0, 256), (4, 3328, 256), (5, 100, 256), (3, 7000, 511), (7, 512, 0)):
        brute = [(u, u * row_stride + i * frame_step) for u in range(n_rows) for i in range(frames_per_row)]
        got = [ref.rows_frame(f, frames_per_row, row_stride, frame_step) for f in range(n_rows * frames_per_row)]
        assert got == brute
        assert ref.rows_staged(n_rows, row_stride, frames_per_row, frame_step, frame_len) == max(o for _, o in brute[-frames_per_row:]) + frame_len
        if frames_per_row % 2 and n_rows > 1:                             # a pair (2p, 2p + 1) of the fast kernel straddles two rows
            assert any(got[f][0] != got[f + 1][0] for f in range(0, len(got) - 1, 2))
