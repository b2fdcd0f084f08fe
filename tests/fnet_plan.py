"""The float32 network's plan restated: parse() in csrc/edison_fnet.hip for .ednf versions 1 and 2, with and without
EDISON_FNET_LARGE / EDISON_FNET_LAYERED, and beside it the layer road's tiling (csrc/fnet.h's ED_FNET_LAYER_* and ws_chunk() in
csrc/edison_fnet.hip). Test infrastructure, not a test: tests/test_fnet_sweep_cpu.py, test_fnet_pad_cpu.py
and test_fnet_large_cpu.py hold the rows of tests/fnet_rows.py to it, the GPU tests hold the loader to it."""
import struct

from edison_amd import cube_import

E_SIZE, E_NO_IMPL = -3, -17          # EDISON_E_SIZE, EDISON_E_NO_IMPL (include/edison_hip.h)
MAX_LAYERS = 16                      # ED_FNET_MAX_LAYERS (csrc/fnet.h)
MAX_BATCH = 16                       # ED_FNET_MAX_BATCH
LDS_BYTES = 160 * 1024               # ED_FNET_LDS_BYTES
MAX_DIM = 4096                       # EDF_MAX_DIM (edison_fnet.hip)

MB, NB, KC = 128, 64, 64                 # ED_FNET_LAYER_MB / _NB / _KC: a workgroup's rows and channels, the K chunk
WAVE_ROWS = 16                           # one M tile per wave
LAYER_LDS_BYTES = 4 * (MB * (KC + 2) + KC * (NB + 16) + 3 * MB)     # ED_FNET_LAYER_LDS_BYTES
WS_DEFAULT = 256 << 20                   # ED_FNET_WORKSPACE_DEFAULT
INT32_MAX = 2 ** 31 - 1


def plan(blob, large=False, layered=False):
    """The kernel plan parse() builds from an .ednf blob: dict(n_layers, in_n, n_out, batch, buf_n, w_lds, k_lds, acts_floats,
    lds_bytes, layered, lifted, layers=[dict(P, rows, K, k_pad, n_pad, NT, NG, nt_last, src, dst, relu, out_c, out_n, in_c, inp, k,
    s, p, pad, cpad, ppad, live (rows that are not absent), kn (ints of its k tables in LDS))]), or dict(error=code) for a blob the
    loader refuses. The checks run in parse()'s order, so the code is the one the loader returns.

    large, layered: EDISON_FNET_LARGE and EDISON_FNET_LAYERED. `large` lifts the two LDS refusals and the MAX_DIM bound on a record's
    in_c; `lifted` names the first refusal it lifted ("weights", "acts" or None). A network it lets through, and any network under
    `layered`, is a layered one: batch 0, lds_bytes the layer kernel's. (The loader then also wants one utterance to fit the
    workspace: chunk_of(p, cap) >= 1.)"""
    if len(blob) < 32 or blob[:4] != b"EDNF":
        return dict(error=E_SIZE)
    ver, nl, in_h, in_w, in_c, n_out, kwb = struct.unpack_from("<7i", blob, 4)
    if ver not in (1, 2):
        return dict(error=E_NO_IMPL)
    ri = 16 if ver == 1 else 24
    if nl < 2 or nl > MAX_LAYERS + 1:
        return dict(error=E_NO_IMPL)
    if min(in_h, in_w, in_c) < 1 or max(in_h, in_w, in_c) > MAX_DIM or kwb < 0 or kwb % 4:
        return dict(error=E_SIZE)
    if in_h * in_w * in_c > 1 << 20:
        return dict(error=E_NO_IMPL)
    off = 32 + nl * ri * 4
    if off + kwb > len(blob):
        return dict(error=E_SIZE)
    off += kwb
    h, w, c = in_h, in_w, in_c
    wfl = tabn = acts = 0
    buf = [h * w * c, 0]
    layers, w_lds, k_lds, lifted = [], 0, 0, None
    for i in range(nl):
        v = list(struct.unpack_from("<%di" % ri, blob, 32 + 4 * ri * i)) + [0] * (24 - ri)
        if v[0] not in (cube_import.T_CONV, cube_import.T_SOFTMAX):
            return dict(error=E_NO_IMPL)
        for j in range(1, (15 if v[0] == cube_import.T_CONV else 6) + 1):
            if v[j] < (0 if j == 11 else 1) or v[j] > MAX_DIM * (16 if j >= 14 or (j == 3 and large) else 1):
                return dict(error=E_SIZE)
        if v[0] == cube_import.T_CONV and (min(v[16:24]) < 0 or max(v[16:24]) > MAX_DIM):
            return dict(error=E_SIZE)
        cur = h * w * c
        if v[1] * v[2] * v[3] != cur:
            return dict(error=E_SIZE)
        if v[0] == cube_import.T_SOFTMAX:
            if i != nl - 1:
                return dict(error=E_NO_IMPL)
            if v[4] * v[5] * v[6] != cur:
                return dict(error=E_SIZE)
            continue
        if i == nl - 1:
            return dict(error=E_NO_IMPL)
        ih, iw, ic, kh, kw, sh, sw, ph, pw = v[1], v[2], v[3], v[7], v[8], v[9], v[10], v[12], v[13]
        (pt, pl, pb, pr), (qt, ql, qb, qr) = v[16:20], v[20:24]
        if max(pt, pb) >= kh or max(pl, pr) >= kw:
            return dict(error=E_NO_IMPL)
        if max(qt, qb) >= ph or max(ql, qr) >= pw:
            return dict(error=E_NO_IMPL)
        if kh > ih + pt + pb or kw > iw + pl + pr:
            return dict(error=E_SIZE)
        oh, ow = (ih + pt + pb - kh) // sh + 1, (iw + pl + pr - kw) // sw + 1
        Ph, Pw = cube_import.pooled_dim(oh, qt, qb, ph), cube_import.pooled_dim(ow, ql, qr, pw)
        if v[4] != Ph or v[5] != Pw:
            return dict(error=E_SIZE)
        if v[4] * v[5] * v[6] * ph * pw > 1 << 20 or kh * kw * ic > 1 << 16:
            return dict(error=E_NO_IMPL)
        P = ph * pw
        if P not in (1, 2, 4):
            return dict(error=E_NO_IMPL)
        if v[11] > 1:
            return dict(error=E_SIZE)
        K, oc = kh * kw * ic, v[6]
        if v[14] != (K + 3) // 4 * 4 or v[15] != (oc + 15) // 16 * 16:
            return dict(error=E_SIZE)
        if len(layers) == MAX_LAYERS:
            return dict(error=E_NO_IMPL)
        k_pad, n_pad = v[14], v[15]
        rows, out_n = v[4] * v[5] * P, v[4] * v[5] * oc
        wl = k_pad * n_pad
        if wl > LDS_BYTES // 4:
            if not large:
                return dict(error=E_NO_IMPL)
            lifted = lifted or "weights"
        pad = any(v[16:24])
        kn = 2 * k_pad if pad else k_pad
        live = sum(qt <= y < qt + oh for y in range(Ph * ph)) * sum(ql <= x < ql + ow for x in range(Pw * pw))
        src = len(layers) & 1
        NT = n_pad // 16
        NG = (NT + 3) // 4
        wfl += wl + n_pad
        tabn += kn + rows
        acts += out_n
        if out_n > 1 << 20 or tabn > 1 << 26 or acts > 1 << 26:
            return dict(error=E_NO_IMPL)
        buf[src ^ 1] = max(buf[src ^ 1], out_n)
        w_lds, k_lds = max(w_lds, wl), max(k_lds, kn)
        layers.append(dict(P=P, rows=rows, K=K, k_pad=k_pad, n_pad=n_pad, NT=NT, NG=NG, nt_last=NT - 4 * (NG - 1), src=src, dst=src ^ 1,
                           relu=v[11], out_c=oc, out_n=out_n, in_c=ic, k=(kh, kw), s=(sh, sw), p=(ph, pw), pad=pad, cpad=(pt, pl, pb, pr),
                           ppad=(qt, ql, qb, qr), live=live, kn=kn, inp=(ih, iw, ic)))
        h, w, c = v[4], v[5], oc
    if not layers or h * w * c != n_out:
        return dict(error=E_SIZE)
    if off + 4 * wfl != len(blob):
        return dict(error=E_SIZE)
    buf_n = [(buf[0] + 3) & ~3, (buf[1] + 3) & ~3]
    fixed, per = 4 * (w_lds + k_lds), 4 * (buf_n[0] + buf_n[1])
    batch = min((LDS_BYTES - fixed) // per, MAX_BATCH)
    if batch < 1:
        if not large:
            return dict(error=E_NO_IMPL)
        lifted = lifted or "acts"
    layered = bool(layered or lifted)
    if layered:
        batch = 0
    if batch * layers[-1]["rows"] > INT32_MAX // 16:
        return dict(error=E_NO_IMPL)
    return dict(n_layers=len(layers), in_n=in_h * in_w * in_c, n_out=n_out, batch=batch, buf_n=buf_n, w_lds=w_lds, k_lds=k_lds,
                acts_floats=acts, lds_bytes=LAYER_LDS_BYTES if layered else 4 * (batch * (buf_n[0] + buf_n[1]) + w_lds) + 4 * k_lds,
                layered=layered, lifted=lifted, layers=layers)


# ---- the layer road's tiling, on a layered plan p ---------------------------------------------------------------------------------------
def chunk_of(p, cap=WS_DEFAULT):
    """ws_chunk(): utterances per chunk under a workspace cap of `cap` bytes; 0 when one utterance does not fit."""
    buf_n = p["buf_n"]
    chunk = min([cap // (4 * (buf_n[0] + buf_n[1])), INT32_MAX // max(buf_n)] + [INT32_MAX // 16 // L["rows"] for L in p["layers"]])
    return chunk - chunk % MB if chunk > MB else chunk


def cap_for(p, chunk):
    """A workspace cap that holds `chunk` utterances of plan p and not one more."""
    return 4 * (p["buf_n"][0] + p["buf_n"][1]) * chunk + 4


def launches(p, n, cap=WS_DEFAULT):
    """(n_layers + 1) * chunks: the kernel launches of one call on n utterances."""
    return (p["n_layers"] + 1) * -(-n // chunk_of(p, cap))
