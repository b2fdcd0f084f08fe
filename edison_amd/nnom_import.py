#!/usr/bin/env python3
"""Convert an NNoM-generated ``weights.h`` into this repo's binary model blob.

The reference ships its trained int8 keyword-spotting network as a generated C
header (``firmware/src/ai/nnom/kws_nnom/weights.h``: ``#define X_KERNEL_0 {…}``
arrays, ``*_SHIFT`` macros and the ``nnom_model_create()`` graph, lines 3-161).
The product on the MI355X consumes *parameters*, not C source, so this tool
parses the header and emits a small self-describing binary (``.ednn``) that the
C-ABI library (``edison_model_load``), the Python host side and the oracle all
read.  Only numbers leave the header: tensors, shifts and the layer list.

Layout decisions taken here (and nowhere else):
  * conv kernels stay OHWI (``w[o][ky][kx][ci]``), exactly as CMSIS-NN indexes
    them (arm_convolve_HWC_q7_basic_nonsquare.c:209-211);
  * the dense matrix is DE-INTERLEAVED from ``arm_fully_connected_q7_opt``'s
    storage order (arm_fully_connected_q7_opt.c:374-473, enabled by
    ``DENSE_WEIGHT_OPT 1`` in nnom_port.h:34) into plain row-major
    ``[out][in]``; the blob's flag word records that this was done.

Blob format (little endian):
  char     magic[8]   = b"EDNNOM1\\0"
  int32    in_h, in_w, in_c
  int32    n_layers
  int32    payload_bytes
  int32    reserved[3]   [0] = 1 (flag word: the dense matrices are de-interleaved)
                         [1] = payload offset of the SOURCE TABLE of a branching graph, 0 for a sequential one
                               (every layer reads its predecessor, the first the network input)
  n_layers x int32[12] records:
     [0] type  1=conv2d  2=maxpool  3=dense  4=softmax  5=dw_conv2d  6=avgpool
     conv2d : [1]=out_ch [2]=kh [3]=kw [4]=sh [5]=sw [6]=bias_lshift [7]=out_rshift
              [8]=flags (bit 0 ReLU tail activation, bit 1 PADDING_SAME)   [9]=weight_off [10]=bias_off [11]=in_ch
     maxpool: [2]=kh [3]=kw [4]=sh [5]=sw [8]=flags (bit 1 PADDING_SAME)
     dense  : [1]=out [6]=bias_lshift [7]=out_rshift [8]=flags (bit 0 ReLU) [9]=weight_off [10]=bias_off [11]=in
              (Flatten() is a no-op on HWC memory and leaves no record)
     softmax: -
     dw_conv2d: as conv2d with [1]=[11]=channels (depth multiplier 1 only: in = out channels); weights stay
              ``w[ky][kx][ch]`` as arm_depthwise_separable_conv_HWC_q7_nonsquare.c:392-393 indexes them
     avgpool: as maxpool, and [7]=output_shift (nnom_avgpool.c:70,99; a generated header cannot set it: always 0)
     add=7 sub=8 mult=9 concat=10 (the merge layers of nnom_matrix.c / nnom_concat.c): [1]=out_ch [7]=output shift
              (0 for concat) [8]=flags (bit 0 ReLU tail activation) [11]=number of inputs
  int8     payload[payload_bytes]   (offsets above index into it)
  source table (branching graphs only; 4-byte aligned inside the payload): per record, in record order, int32 n followed by
              n int32 record indices the layer reads, in the order of the merge statement; -1 is the network input. Every
              index points backwards, every record but the last is read by a later one.

Merge layers are accepted where the reference computes what the layer's name says: Add over two or more inputs (the third
and later ones accumulate into the output, nnom_matrix.c:123-137), Sub and Mult over exactly two, Concat over the channel
axis of inputs of one shape (concat_build sizes the output as n times the FIRST input's channels and concat_run copies the
first input's channel count from every input, nnom_concat.c:95-103,197-214: with unequal channel counts that is no
concatenation, and such a graph is refused by name).

Usage:  tools/import_weights_h.py /path/to/weights.h edison_amd/data/kws_nnom.ednn
"""
import re
import struct
import sys

import numpy as np

MAGIC = b"EDNNOM1\0"
T_CONV, T_POOL, T_DENSE, T_SOFTMAX, T_DWCONV, T_AVGPOOL = 1, 2, 3, 4, 5, 6
T_ADD, T_SUB, T_MULT, T_CONCAT = 7, 8, 9, 10
MERGES = {"Add": T_ADD, "Sub": T_SUB, "Mult": T_MULT, "Concat": T_CONCAT}
# layers of nnom_layers.h this importer names when it refuses them (the reference runs them, this path does not)
REFUSED = ("GlobalMaxPool", "GlobalAvgPool", "GlobalSumPool", "SumPool", "ZeroPadding", "Cropping", "UpSample", "Lambda", "RNN", "Activation", "ReLU", "Sigmoid", "TanH", "BaseLayer")


def _eval_int(expr, sym):
    """Evaluate a +/- expression of integer literals and already known macros."""
    def repl(m):
        name = m.group(0)
        if name not in sym:
            raise KeyError("unknown macro %s in %r" % (name, expr))
        return str(sym[name])
    flat = re.sub(r"[A-Za-z_]\w*", repl, expr)
    if not re.fullmatch(r"[\d\s()+\-]+", flat):
        raise ValueError("unsupported macro expression %r" % expr)
    return int(eval(flat, {"__builtins__": {}}))  # digits, + - ( ) only (checked above)


def parse_weights_h(text):
    """Return (input_shape, layers, arrays) parsed from the text of a weights.h."""
    arrays, sym, pending = {}, {}, []
    for m in re.finditer(r"#define\s+(\w+)\s+\{([^}]*)\}", text):
        arrays[m.group(1)] = np.array([int(v) for v in m.group(2).replace("\n", " ").split(",") if v.strip()],
                                      dtype=np.int64)
    for m in re.finditer(r"^#define\s+(\w+)\s+(\(?[^{}\n]+?\)?)\s*$", text, flags=re.M):
        name, expr = m.group(1), m.group(2).strip()
        if name in arrays:
            continue
        pending.append((name, expr))
    # macros may reference later ones; iterate to a fixed point
    for _ in range(8):
        rest = []
        for name, expr in pending:
            try:
                sym[name] = _eval_int(expr, sym)
            except (KeyError, ValueError):
                rest.append((name, expr))
        if not rest or len(rest) == len(pending):
            break
        pending = rest

    # static const int8_t conv2d_1_weights[] = CONV2D_1_KERNEL_0;
    c_arrays = {m.group(1): m.group(2) for m in
                re.finditer(r"static const int8_t\s+(\w+)\[\]\s*=\s*(\w+);", text)}
    # static const nnom_weight_t conv2d_1_w = { (const void*)conv2d_1_weights, CONV2D_1_OUTPUT_RSHIFT};
    structs = {m.group(1): (m.group(2), m.group(3)) for m in
               re.finditer(r"static const nnom_(?:weight|bias)_t\s+(\w+)\s*=\s*\{\s*\(const void\*\)\s*(\w+)\s*,\s*(\w+)\s*\}",
                           text)}

    def tensor(struct_name):
        arr_name, shift_name = structs[struct_name]
        vals = arrays[c_arrays[arr_name]]
        if vals.min() < -128 or vals.max() > 127:
            raise ValueError("%s does not fit int8" % arr_name)
        return vals.astype(np.int8), int(sym[shift_name])

    m = re.search(r"Input\(shape\((\d+),\s*(\d+),\s*(\d+)\)", text)
    if not m:
        raise ValueError("no Input(shape(h,w,c)) in weights.h")
    in_shape = tuple(int(g) for g in m.groups())

    layers = []
    rec_of = {}       # header layer[k] -> record index; -1 is the network input (Input, or a Flatten / Output of it)
    out_rec = None    # the record the Output layer hooks
    shapes = []       # (h, w, c) of every record's output
    dim = {"PADDING_VALID": 0, "PADDING_SAME": 1}

    def source(line, k):
        """Record index the hooked / activated layer[j] of a statement stands for."""
        j = int(re.findall(r"layer\[(\d+)\]", line)[-1])
        if j not in rec_of or j >= k:
            raise ValueError("layer[%d] reads layer[%d], which is not built before it: %s" % (k, j, line))
        return rec_of[j]

    def shape_of(r):
        return in_shape if r < 0 else shapes[r]

    def add(k, src, shape, **fields):
        layers.append(dict(src=list(src), **fields))
        shapes.append(tuple(shape))
        rec_of[k] = len(layers) - 1

    for k, line in re.findall(r"layer\[(\d+)\]\s*=\s*(.*);", text):
        k = int(k)
        mw = re.search(r"\bDW_Conv2D\((\d+),\s*kernel\((\d+),\s*(\d+)\),\s*stride\((\d+),\s*(\d+)\),\s*(\w+),\s*&(\w+),\s*&(\w+)\)", line)
        ma = re.search(r"\bAvgPool\(kernel\((\d+),\s*(\d+)\),\s*stride\((\d+),\s*(\d+)\),\s*(\w+)\)", line)
        refused = re.search(r"\b(%s)\(" % "|".join(REFUSED), line)
        mc = None if mw else re.search(r"\bConv2D\((\d+),\s*kernel\((\d+),\s*(\d+)\),\s*stride\((\d+),\s*(\d+)\),\s*(\w+),\s*&(\w+),\s*&(\w+)\)", line)
        mp = re.search(r"\bMaxPool\(kernel\((\d+),\s*(\d+)\),\s*stride\((\d+),\s*(\d+)\),\s*(\w+)\)", line)
        md = re.search(r"\bDense\((\d+),\s*&(\w+),\s*&(\w+)\)", line)
        mm = re.search(r"\bmodel\.(merge|mergex)\(\s*(Add|Sub|Mult|Concat)\(([^()]*)\)\s*,(.*)\)\s*$", line)
        if refused:
            raise ValueError("unsupported layer %s in weights.h: %s" % (refused.group(1), line))
        if mm:
            name, arg, rest = mm.group(2), mm.group(3).strip(), mm.group(4)
            ins = [int(j) for j in re.findall(r"layer\[(\d+)\]", rest)]
            if mm.group(1) == "mergex":
                count = _eval_int(rest.split(",")[0], sym)
                if count != len(ins):
                    raise ValueError("%s: mergex names %d inputs and lists %d: %s" % (name, count, len(ins), line))
            for j in ins:
                if j not in rec_of or j >= k:
                    raise ValueError("%s: layer[%d] reads layer[%d], which is not built before it: %s" % (name, k, j, line))
            src = [rec_of[j] for j in ins]
            if len(src) < 2:
                raise ValueError("%s needs two inputs or more: %s" % (name, line))
            if name in ("Sub", "Mult") and len(src) != 2:
                raise ValueError("%s over %d inputs: the reference's loop for a third input (nnom_matrix.c:159-207) does not "
                                 "compute a %s; exactly two are supported" % (name, len(src), name))
            first = shape_of(src[0])
            for r in src[1:]:
                if shape_of(r) != first:
                    raise ValueError("%s: inputs of unequal shape %s and %s (Concat included: the reference copies the first "
                                     "input's channel count from every input, nnom_concat.c:197-214)" % (name, first, shape_of(r)))
            if name == "Concat":
                axis = _eval_int(arg, sym)
                if axis not in (-1, 3):
                    raise ValueError("Concat on axis %d: only the channel axis (-1 or 3) is supported" % axis)
                add(k, src, (first[0], first[1], first[2] * len(src)), type=T_CONCAT, out_shift=0, relu=0)
            else:
                shift = _eval_int(arg, sym)
                if not 0 <= shift <= 15:
                    raise ValueError("%s: output shift %d out of range" % (name, shift))
                add(k, src, first, type=MERGES[name], out_shift=shift, relu=0)
            continue
        if "Input(" in line:
            rec_of[k] = -1
            continue
        if "act_relu()" in line:
            r = source(line, k)
            if r < 0 or layers[r]["type"] not in (T_CONV, T_DENSE, T_DWCONV, T_ADD, T_SUB, T_MULT, T_CONCAT):
                raise ValueError("ReLU tail activation is only supported after Conv2D, DW_Conv2D, Dense, Add, Sub, Mult or Concat")
            layers[r]["relu"] = 1
            rec_of[k] = r
            continue
        s0 = source(line, k)
        h, w_, c = shape_of(s0)
        if mw:
            # nnom_dw_conv2d.c:88-89: with CMSIS-NN the reference returns NN_ARGUMENT_ERROR for these
            if int(mw.group(1)) != 1:
                raise ValueError("DW_Conv2D with depth multiplier %s: the reference's CMSIS-NN build runs multiplier 1 only" % mw.group(1))
            if c % 2:
                raise ValueError("DW_Conv2D over %d channels: the reference's CMSIS-NN build refuses an odd channel count" % c)
            if mw.group(6) not in dim:
                raise ValueError("DW_Conv2D: unknown padding %s" % mw.group(6))
            w, rs = tensor(mw.group(7))
            b, bl = tensor(mw.group(8))
            kh, kw, sh, sw, same = int(mw.group(2)), int(mw.group(3)), int(mw.group(4)), int(mw.group(5)), dim[mw.group(6)]
            if w.size != kh * kw * c or b.size != c:
                raise ValueError("DW_Conv2D: %d weights and %d biases for a %dx%d kernel over %d channels" % (w.size, b.size, kh, kw, c))
            add(k, [s0], (out_dim(h, kh, sh, same), out_dim(w_, kw, sw, same), c), type=T_DWCONV, kh=kh, kw=kw, sh=sh, sw=sw, w=w, b=b,
                out_rshift=rs, bias_lshift=bl, relu=0, same=same)
        elif ma or mp:
            m2, what = (ma, "AvgPool") if ma else (mp, "MaxPool")
            if m2.group(5) not in dim:
                raise ValueError("%s: unknown padding %s" % (what, m2.group(5)))
            kh, kw, sh, sw, same = int(m2.group(1)), int(m2.group(2)), int(m2.group(3)), int(m2.group(4)), dim[m2.group(5)]
            extra = dict(out_shift=0) if ma else {}
            add(k, [s0], (out_dim(h, kh, sh, same), out_dim(w_, kw, sw, same), c), type=T_AVGPOOL if ma else T_POOL, kh=kh, kw=kw,
                sh=sh, sw=sw, same=same, **extra)
        elif mc:
            if mc.group(6) not in dim:
                raise ValueError("unknown padding %s" % mc.group(6))
            w, rs = tensor(mc.group(7))
            b, bl = tensor(mc.group(8))
            kh, kw, sh, sw, same = int(mc.group(2)), int(mc.group(3)), int(mc.group(4)), int(mc.group(5)), dim[mc.group(6)]
            add(k, [s0], (out_dim(h, kh, sh, same), out_dim(w_, kw, sw, same), int(mc.group(1))), type=T_CONV, out_ch=int(mc.group(1)),
                kh=kh, kw=kw, sh=sh, sw=sw, w=w, b=b, out_rshift=rs, bias_lshift=bl, relu=0, same=same)
        elif md:
            w, rs = tensor(md.group(2))
            b, bl = tensor(md.group(3))
            add(k, [s0], (1, 1, int(md.group(1))), type=T_DENSE, out=int(md.group(1)), w=w, b=b, out_rshift=rs, bias_lshift=bl, relu=0)
        elif "Softmax()" in line:
            add(k, [s0], (h, w_, c), type=T_SOFTMAX)
        elif "Output(" in line or "Flatten()" in line:
            rec_of[k] = s0
            if "Output(" in line:
                out_rec = s0
        else:
            raise ValueError("unsupported layer in weights.h: %s" % line)
    # the network's output is the last record's: an Output hooked to an earlier one would be answered with another tensor
    if out_rec is not None and out_rec != len(layers) - 1:
        raise ValueError("Output reads record %d, not the last record %d: nothing reads the output of the records behind it"
                         % (out_rec, len(layers) - 1))
    read = {r for L in layers for r in L["src"]}
    for i in range(len(layers) - 1):
        if i not in read:
            raise ValueError("record %d (type %d): nothing reads its output" % (i, layers[i]["type"]))
    return in_shape, layers


def deinterleave_dense_opt(stream, rows, cols):
    """Invert arm_fully_connected_q7_opt's weight order (portable branch,
    arm_fully_connected_q7_opt.c:374-473): rows in groups of 4, columns in groups
    of 4, 16 bytes per (row-group, column-block); leftover columns of a row group
    follow as 4 bytes (one per row); leftover rows follow plain row-major."""
    w = np.zeros((rows, cols), dtype=np.int8)
    p = 0
    # byte i of a 16-byte block -> (row offset, column offset)
    blk = [(0, 0), (1, 0), (0, 2), (1, 2), (2, 0), (3, 0), (2, 2), (3, 2),
           (0, 1), (1, 1), (0, 3), (1, 3), (2, 1), (3, 1), (2, 3), (3, 3)]
    for r in range(0, rows - rows % 4, 4):
        for c in range(0, cols - cols % 4, 4):
            for i, (dr, dc) in enumerate(blk):
                w[r + dr, c + dc] = stream[p + i]
            p += 16
        for c in range(cols - cols % 4, cols):
            for dr in range(4):
                w[r + dr, c] = stream[p]
                p += 1
    for r in range(rows - rows % 4, rows):
        w[r, :] = stream[p:p + cols]
        p += cols
    assert p == rows * cols
    return w


def out_dim(n, k, s, same):
    """NN_CEILIF(n, s) for PADDING_SAME, NN_CEILIF(n - k + 1, s) otherwise (nnom_conv2d.c:92-104)."""
    return -(-n // s) if same else -(-(n - k + 1) // s)


def build_blob(in_shape, layers, dense_plain=False):
    """dense_plain: the dense matrices are already plain row-major [out][in] (edison_amd/quantize.py), not in
    arm_fully_connected_q7_opt's storage order; the blob is the same either way."""
    payload = bytearray()
    records = []
    shapes = []   # every record's output; a layer without "src" reads its predecessor

    def put(arr):
        # keep every tensor 16-byte aligned inside the payload
        while len(payload) % 16:
            payload.append(0)
        off = len(payload)
        payload.extend(np.ascontiguousarray(arr, dtype=np.int8).tobytes())
        return off

    srcs = []
    for i, L in enumerate(layers):
        src = list(L.get("src", [i - 1]))
        for r in src:
            if not -1 <= r < i:
                raise ValueError("record %d reads record %d: a source must point backwards" % (i, r))
        srcs.append(src)
        h, w_, c = in_shape if src[0] < 0 else shapes[src[0]]
        rec = [0] * 12
        rec[0] = L["type"]
        if L["type"] == T_CONV:
            k = L["kh"] * L["kw"] * c
            assert L["w"].size == L["out_ch"] * k, "conv weight size mismatch"
            rec[1:9] = [L["out_ch"], L["kh"], L["kw"], L["sh"], L["sw"], L["bias_lshift"], L["out_rshift"],
                        L["relu"] | (L["same"] << 1)]
            rec[9], rec[10], rec[11] = put(L["w"]), put(L["b"]), c
            h, w_, c = out_dim(h, L["kh"], L["sh"], L["same"]), out_dim(w_, L["kw"], L["sw"], L["same"]), L["out_ch"]
        elif L["type"] == T_DWCONV:
            if c % 2:
                raise ValueError("DW_Conv2D over %d channels: the reference's CMSIS-NN build refuses an odd channel count" % c)
            if L["w"].size != L["kh"] * L["kw"] * c or L["b"].size != c:
                raise ValueError("DW_Conv2D: %d weights and %d biases for a %dx%d kernel over %d channels"
                                 % (L["w"].size, L["b"].size, L["kh"], L["kw"], c))
            rec[1:9] = [c, L["kh"], L["kw"], L["sh"], L["sw"], L["bias_lshift"], L["out_rshift"], L["relu"] | (L["same"] << 1)]
            rec[9], rec[10], rec[11] = put(L["w"]), put(L["b"]), c
            h, w_ = out_dim(h, L["kh"], L["sh"], L["same"]), out_dim(w_, L["kw"], L["sw"], L["same"])
        elif L["type"] == T_AVGPOOL:
            if L.get("out_shift", 0) != 0:
                raise ValueError("AvgPool with output_shift %d: only 0 is supported" % L["out_shift"])
            rec[2:6] = [L["kh"], L["kw"], L["sh"], L["sw"]]
            rec[7], rec[8] = 0, L["same"] << 1
            h, w_ = out_dim(h, L["kh"], L["sh"], L["same"]), out_dim(w_, L["kw"], L["sw"], L["same"])
        elif L["type"] == T_POOL:
            rec[2:6] = [L["kh"], L["kw"], L["sh"], L["sw"]]
            rec[8] = L["same"] << 1
            h, w_ = out_dim(h, L["kh"], L["sh"], L["same"]), out_dim(w_, L["kw"], L["sw"], L["same"])
        elif L["type"] == T_DENSE:
            n_in = h * w_ * c
            assert L["w"].size == L["out"] * n_in, "dense weight size mismatch"
            plain = np.asarray(L["w"], np.int8).reshape(L["out"], n_in) if dense_plain else deinterleave_dense_opt(L["w"], L["out"], n_in)
            rec[1], rec[6], rec[7], rec[8] = L["out"], L["bias_lshift"], L["out_rshift"], L["relu"]
            rec[9], rec[10], rec[11] = put(plain), put(L["b"]), n_in
            h, w_, c = 1, 1, L["out"]
        elif L["type"] in (T_ADD, T_SUB, T_MULT, T_CONCAT):
            name = {T_ADD: "Add", T_SUB: "Sub", T_MULT: "Mult", T_CONCAT: "Concat"}[L["type"]]
            if len(src) < 2 or (L["type"] in (T_SUB, T_MULT) and len(src) != 2):
                raise ValueError("%s over %d inputs" % (name, len(src)))
            for r in src[1:]:
                if (in_shape if r < 0 else shapes[r]) != (h, w_, c):
                    raise ValueError("%s: inputs of unequal shape" % name)
            if L["type"] == T_CONCAT:
                c *= len(src)
            rec[1], rec[7], rec[8], rec[11] = c, L.get("out_shift", 0), L.get("relu", 0), len(src)
        shapes.append((h, w_, c))
        records.append(rec)
    table_off = 0
    if any(src != [i - 1] for i, src in enumerate(srcs)):
        read = {r for src in srcs for r in src}
        for i in range(len(layers) - 1):
            if i not in read:
                raise ValueError("record %d: nothing reads its output" % i)
        while len(payload) % 16 or not payload:
            payload.append(0)
        table_off = len(payload)
        payload.extend(np.array([v for src in srcs for v in [len(src)] + src], dtype="<i4").tobytes())
    while len(payload) % 16:
        payload.append(0)
    head = MAGIC + struct.pack("<8i", in_shape[0], in_shape[1], in_shape[2], len(records), len(payload), 1, table_off, 0)
    body = b"".join(struct.pack("<12i", *r) for r in records)
    return head + body + bytes(payload)


def blob_sources(blob):
    """Per record, the record indices it reads (-1: the network input), from a blob's source table or its absence."""
    head = struct.unpack_from("<8i", blob, 8)
    n, off = head[3], head[6]
    if off == 0:
        return [[i - 1] for i in range(n)]
    pay = 40 + 48 * n + off
    out = []
    for _ in range(n):
        cnt = struct.unpack_from("<i", blob, pay)[0]
        out.append(list(struct.unpack_from("<%di" % cnt, blob, pay + 4)))
        pay += 4 * (cnt + 1)
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    with open(argv[1], "r") as f:
        text = f.read()
    in_shape, layers = parse_weights_h(text)
    blob = build_blob(in_shape, layers)
    with open(argv[2], "wb") as f:
        f.write(blob)
    print("wrote %s: input %s, %d layers, %d bytes" % (argv[2], in_shape, len(layers), len(blob)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
