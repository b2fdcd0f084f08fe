"""The firmware's NNoM keyword-spotting example (appNnomKwsRun, firmware/src/app.c:545-623) and nnom_predict's result rule
(nnom_utils.c:258-305), restated in numpy. Test infrastructure, not a test: tests/test_nnom_kws_cpu.py checks it on the CPU,
tests/test_gpu_nnom_kws.py compares the GPU entry points with it.

The loop, per audio event of 512 new samples (AUDIO_FRAME_LEN):
    audio_buffer_16bit [768]: the last 256 samples move to the front, the 512 new ones go behind them       (app.c:567-575)
    two frames of 512 samples at offsets 0 and 256 go through mfcc_compute into the ring mfcc_features[rows] at mfcc_feat_index,
    which wraps at `rows` (MFCC_LEN)                                                                            (app.c:581-596)
    mfcc_features_seq = the ring unrolled from mfcc_feat_index, i.e. oldest row first                           (app.c:600-604)
    aiNnomPredict on mfcc_features_seq                                                                           (app.c:612-613)
All buffers are static, so they start as zeros. The feature function is an argument: frame [512] int16 -> row [n_out] int8.
"""
import numpy as np

EVENT = 512      # AUDIO_FRAME_LEN, app.c:497
HALF = 256       # the 50 % overlap, app.c:583


def ring_loop(feature_fn, samples, rows, n_out):
    """The windows mfcc_features_seq holds after every event: int8 [n_events, rows, n_out]"""
    x = np.ascontiguousarray(samples, dtype=np.int16).ravel()
    assert x.size % EVENT == 0
    buf = np.zeros(EVENT + HALF, np.int16)                 # audio_buffer_16bit
    ring = np.zeros((rows, n_out), np.int8)                # mfcc_features
    idx, out = 0, []                                       # mfcc_feat_index
    for e in range(x.size // EVENT):
        buf[:HALF] = buf[EVENT:EVENT + HALF].copy()
        buf[HALF:] = x[e * EVENT:(e + 1) * EVENT]
        for i in range(2):
            ring[idx] = feature_fn(buf[i * HALF:i * HALF + EVENT])
            idx += 1
            if idx >= rows:
                idx = 0
        len_second = idx * n_out
        flat = ring.reshape(-1)
        out.append(np.concatenate([flat[len_second:], flat[:len_second]]).reshape(rows, n_out))
    return np.stack(out) if out else np.zeros((0, rows, n_out), np.int8)


def row_sequence(feature_fn, samples, n_out):
    """Every feature row the loop computes, in time order: row r is the frame at sample 256 r of [256 zeros | samples]; [2 n_events, n_out]"""
    x = np.concatenate([np.zeros(HALF, np.int16), np.ascontiguousarray(samples, dtype=np.int16).ravel()])
    n = 2 * ((x.size - HALF) // EVENT)
    return np.stack([feature_fn(x[r * HALF:r * HALF + EVENT]) for r in range(n)]) if n else np.zeros((0, n_out), np.int8)


def sliding_windows(seq, rows):
    """The sliding form: window e = rows 2e + 2 - rows .. 2e + 1 of the row sequence, rows before the start being zero bytes. It is what
    a buffer [rows zero rows | seq] gives when window e is read in place from row 2e + 2 on."""
    padded = np.concatenate([np.zeros((rows, seq.shape[1]), seq.dtype), seq])
    return np.stack([padded[2 * e + 2:2 * e + 2 + rows] for e in range(seq.shape[0] // 2)]) if seq.shape[0] else np.zeros((0, rows, seq.shape[1]), seq.dtype)


def predict_rule(out):
    """nnom_predict on int8 [n, n_out]: (label uint32 [n], prob float32 [n]). n_out > 1: the first strict maximum, max / sum in float32
    with the int32 sum over all values, 0 when the sum is 0 (nnom_utils.c:272-293); n_out == 1: out / 127.f, label = prob >= 0.5f
    (nnom_utils.c:295-302)."""
    o = np.asarray(out, dtype=np.int8)
    n, n_out = o.shape
    label, prob = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    for i in range(n):
        if n_out > 1:
            max_val, max_index, s = int(o[i, 0]), 0, int(o[i, 0])
            for j in range(1, n_out):
                if int(o[i, j]) > max_val:
                    max_val, max_index = int(o[i, j]), j
                s += int(o[i, j])
            label[i] = max_index
            prob[i] = np.float32(max_val) / np.float32(s) if s != 0 else np.float32(0)
        else:
            prob[i] = np.float32(int(o[i, 0])) / np.float32(127.0)
            label[i] = 1 if prob[i] >= np.float32(0.5) else 0
    return label, prob


def rows_frame(f, frames_per_row, row_stride, frame_step):
    """The rows form of variant D: (row, sample offset) of frame f"""
    u = f // frames_per_row
    return u, u * row_stride + (f % frames_per_row) * frame_step


def rows_staged(n_rows, row_stride, frames_per_row, frame_step, frame_len):
    """Samples a host call of the rows form stages"""
    return (n_rows - 1) * row_stride + (frames_per_row - 1) * frame_step + frame_len
