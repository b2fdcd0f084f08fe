"""tests/dscnn_ref.py -- TEST INFRASTRUCTURE: numpy restatement of NNoM 0.3.0's DW_Conv2D and AvgPool (CMSIS-NN on, HWC,
portable branches), written from the reference's sources and independent of the product's kernels and planner. The layers
oracle/net_ref.py already restates are run by it: a graph is cut into runs of old layers (handed to net_ref.run as a blob
of their own) and the two new layers between them. Pinned by tests/golden/dscnn_golden.npz (gen_fixtures_dscnn.py).

  DW_Conv2D  per output pixel and channel: conv_out = (bias << bias_shift) + NN_ROUND(out_shift), plus x * w over the taps
             inside the image, w indexed [ky][kx][ch]; out = sat8(conv_out >> out_shift)
             (arm_depthwise_separable_conv_HWC_q7_nonsquare.c:376-401); padding (k-1)/2 under PADDING_SAME, output
             ceil(in/stride) or ceil((in-k+1)/stride) (nnom_conv2d.c:66-71, nnom_dw_conv2d.c:56-67); ReLU as a tail activation
  AvgPool    sum over the taps inside the image, divided by their number with C's `/` (truncation toward zero), stored as int8:
             local_avepool_q7_HWC (nnom_local.c:45-67, `sum / (count >> output_shift)`, output_shift = 0) and the portable branch
             of arm_avepool_q7_HWC (arm_pool_q7_HWC.c:424-446, `sum / count`) divide the same way. What differs is the WINDOW:
             when the input and the output are both square, avgpool_run (nnom_avgpool.c:76-86) calls the CMSIS routine with
             kernel.w, pad.w and stride.w only, and the routine uses them on both axes; otherwise the local routine gets both
             axes' own numbers. Output size and padding are MaxPool's (nnom_maxpool.c:65-104).

`wrong` names one deliberate mis-reading, for the tests that show the fixture tells them apart:
  floor_div      Python's floor division instead of C's truncation
  count_area     divide by kh * kw instead of the number of taps inside the image
  no_round       DW_Conv2D without NN_ROUND(out_shift)
  chw_weights    DW_Conv2D weights read as [ch][ky][kx]
  cmsis_always   the square routine's window rule (kernel.w for both axes) on every AvgPool
  local_always   the stated window on every AvgPool, square maps included
"""
import struct

import numpy as np

from oracle import net_ref

T_DWCONV, T_AVGPOOL = 5, 6


def _out_dim(n, k, s, same):
    return -(-n // s) if same else -(-(n - k + 1) // s)


def dw_conv2d(x, wt, bias, kh, kw, sh, sw, same, bias_shift, out_shift, relu, wrong=None):
    """x (n, h, w, c) int -> (n, oh, ow, c) int8 values as int32."""
    n, h, w, c = x.shape
    ph, pw = ((kh - 1) // 2, (kw - 1) // 2) if same else (0, 0)
    oh, ow = _out_dim(h, kh, sh, same), _out_dim(w, kw, sw, same)
    wt = np.asarray(wt, dtype=np.int64)
    wt = wt.reshape(c, kh, kw).transpose(1, 2, 0) if wrong == "chw_weights" else wt.reshape(kh, kw, c)
    rnd = 0 if wrong == "no_round" else (1 << out_shift) >> 1
    out = np.zeros((n, oh, ow, c), dtype=np.int64)
    for oy in range(oh):
        for ox in range(ow):
            acc = np.broadcast_to((np.asarray(bias, dtype=np.int64) << bias_shift) + rnd, (n, c)).copy()
            for ky in range(kh):
                for kx in range(kw):
                    iy, ix = sh * oy + ky - ph, sw * ox + kx - pw
                    if 0 <= iy < h and 0 <= ix < w:
                        acc += x[:, iy, ix, :].astype(np.int64) * wt[ky, kx]
            out[:, oy, ox, :] = np.clip(acc >> out_shift, -128, 127)
    if relu:
        out = np.maximum(out, 0)
    return out.astype(np.int32)


def avgpool(x, kh, kw, sh, sw, same, wrong=None):
    n, h, w, c = x.shape
    ph, pw = ((kh - 1) // 2, (kw - 1) // 2) if same else (0, 0)
    oh, ow = _out_dim(h, kh, sh, same), _out_dim(w, kw, sw, same)
    square = h == w and oh == ow
    if (square and wrong != "local_always") or wrong == "cmsis_always":
        kh, ph, sh = kw, pw, sw                     # arm_avepool_q7_HWC(.., cl->kernel.w, cl->pad.w, cl->stride.w, ..)
    out = np.zeros((n, oh, ow, c), dtype=np.int64)
    for oy in range(oh):
        for ox in range(ow):
            s = np.zeros((n, c), dtype=np.int64)
            count = 0
            for iy in range(oy * sh - ph, oy * sh - ph + kh):
                for ix in range(ox * sw - pw, ox * sw - pw + kw):
                    if 0 <= iy < h and 0 <= ix < w:
                        s += x[:, iy, ix, :]
                        count += 1
            d = kh * kw if wrong == "count_area" else count
            q = s // d if wrong == "floor_div" else np.sign(s) * (np.abs(s) // d)
            out[:, oy, ox, :] = q
    return out.astype(np.int8).astype(np.int32)     # the C store into q7_t (|q| <= 128 cannot wrap: |sum| <= 128 * count)


def run(blob, x, wrong=None):
    """As oracle.net_ref.run: dict(acts=[per-layer (n, out_n) int8], logits, softmax (or None), argmax)."""
    (h, w, c), recs, payload = net_ref.parse_blob(blob)
    x = np.ascontiguousarray(x, dtype=np.int8).reshape(-1, h * w * c)
    n = x.shape[0]
    cur = x
    acts = []
    has_softmax = False
    i = 0
    while i < len(recs):
        v = recs[i]
        if v[0] in (T_DWCONV, T_AVGPOOL):
            kh, kw, sh, sw, same = v[2], v[3], v[4], v[5], (v[8] >> 1) & 1
            img = cur.reshape(n, h, w, c).astype(np.int32)
            if v[0] == T_DWCONV:
                assert v[1] == c and v[11] == c
                out = dw_conv2d(img, payload[v[9]:v[9] + kh * kw * c], payload[v[10]:v[10] + c], kh, kw, sh, sw, same, v[6], v[7], v[8] & 1, wrong)
            else:
                assert v[7] == 0, "AvgPool output_shift"
                out = avgpool(img, kh, kw, sh, sw, same, wrong)
            h, w = out.shape[1], out.shape[2]
            cur = out.reshape(n, -1).astype(np.int8)
            acts.append(cur)
            i += 1
            continue
        j = i
        while j < len(recs) and recs[j][0] not in (T_DWCONV, T_AVGPOOL):
            j += 1
        # the old layers i .. j-1 as a graph of their own over the current tensor: same payload, same records
        sub = (b"EDNNOM1\0" + struct.pack("<8i", h, w, c, j - i, payload.size, 1, 0, 0) +
               b"".join(struct.pack("<12i", *recs[k]) for k in range(i, j)) + payload.tobytes())
        r = net_ref.run(sub, cur)
        acts.extend(r["acts"])
        cur = r["acts"][-1]
        for k in range(i, j):
            t = recs[k]
            if t[0] in (net_ref.T_CONV, net_ref.T_POOL):
                same = (t[8] >> 1) & 1
                h, w = _out_dim(h, t[2], t[4], same), _out_dim(w, t[3], t[5], same)
                if t[0] == net_ref.T_CONV:
                    c = t[1]
            elif t[0] == net_ref.T_DENSE:
                h, w, c = 1, 1, t[1]
            elif t[0] == net_ref.T_SOFTMAX:
                has_softmax = True
        i = j
    last = acts[-1]
    return dict(acts=acts, logits=acts[-2] if has_softmax else last, softmax=last if has_softmax else None,
                argmax=np.argmax(last, axis=1).astype(np.int32))
