"""Write a float32 network in X-CUBE-AI's generated-source format (<net>.c declarations + <net>_data.c weight bytes, as
firmware/src/ai/cube/kws/kws.c and kws_data.c are laid out) from seeded random weights: the importer's input for networks at other
geometries than the shipped one, and for layers it must refuse.

Layer specs: ("conv", out_c, (kh, kw), (sh, sw), (ph, pw), relu[, cpad, ppad]) -- conv2d_nl_pool when (ph, pw) != (1, 1), else
conv2d; the pads (top, left, bottom, right), zeros when left out, are written as X-CUBE-AI's (x start, y start, x end, y end) --
("dense", n_out), ("relu",), ("softmax",). weight_scale: the conv weights' deviation in place of 1 / sqrt(K); overrides: {layer name:
fields of its layer declaration to replace}; declared: {layer index: (h, w)} writes another output shape than the computed one. The
last two are for sources the importer must refuse. Returns (net_c, data_c)."""
import numpy as np

from edison_amd import cube_import

from fnet_host import Z4, out_hw


def _hwc(name, h, w, c, array=None):
    return dict(name=name, shape=(1, c, w, h), stride=(4, 4, 4 * c, 4 * c * w), array=array or name + "_array", n=h * w * c)


def cube_sources(in_shape, specs, seed=0, name="net", weight_scale=None, overrides=None, declared=None):
    rng = np.random.default_rng(seed)
    overrides = overrides or {}
    h, w, c = in_shape
    tensors, arrays, layers, blob, woff = [], {}, [], bytearray(), {}
    t_in = _hwc("input_0_output", h, w, c)
    tensors.append(t_in)
    arrays[t_in["array"]] = (t_in["n"], "AI_ARRAY_FORMAT_FLOAT|AI_FMT_FLAG_IS_IO")
    cur = t_in

    def add_weights(tname, shape, stride, vals):
        arr = tname + "_array"
        tensors.append(dict(name=tname, shape=shape, stride=stride, array=arr, n=vals.size))
        arrays[arr] = (vals.size, "AI_ARRAY_FORMAT_FLOAT")
        woff[arr] = len(blob)
        blob.extend(np.asarray(vals, "<f4").tobytes())
        return tname

    def shape4(p):
        return "AI_SHAPE_INIT(4, %d, %d, %d, %d)" % (p[1], p[0], p[3], p[2])

    for i, s in enumerate(specs):
        lname = "layer_%d" % i
        if s[0] == "conv":
            _, oc, (kh, kw), (sh, sw), (ph, pw), relu, cp, pp = s if len(s) == 8 else s + (Z4, Z4)
            ic = cur["shape"][1]
            ch, cw = cur["shape"][3], cur["shape"][2]
            oh, ow = (declared or {}).get(i) or out_hw((ch, cw), (kh, kw), (sh, sw), (ph, pw), cp, pp)
            sc = weight_scale or 1.0 / np.sqrt(kh * kw * ic)
            W = rng.normal(0, sc, (oc, kh, kw, ic)).astype(np.float32)       # [out][kh][kw][in]
            B = rng.normal(0, 0.1, oc).astype(np.float32)
            wt = add_weights(lname + "_weights", (ic, kw, kh, oc), (4, 4 * ic, 4 * ic * kw, 4 * ic * kw * kh), W.reshape(-1))
            bt = add_weights(lname + "_bias", (1, oc, 1, 1), (4, 4, 4 * oc, 4 * oc), B)
            out = _hwc(lname + "_output", oh, ow, oc)
            pool = (ph, pw) != (1, 1)
            fields = [".groups = 1", ".nl_func = %s" % ("nl_func_relu_array_f32" if relu else "NULL"),
                      ".filter_stride = AI_SHAPE_2D_INIT(%d, %d)" % (sw, sh), ".dilation = AI_SHAPE_2D_INIT(1, 1)",
                      ".filter_pad = " + shape4(cp)]
            if pool:
                fields += [".pool_size = AI_SHAPE_2D_INIT(%d, %d)" % (pw, ph), ".pool_stride = AI_SHAPE_2D_INIT(%d, %d)" % (pw, ph),
                           ".pool_pad = " + shape4(pp), ".pool_func = pool_func_mp_array_f32"]
            kind = ("OPTIMIZED_CONV2D_TYPE", "conv2d_nl_pool", "forward_conv2d_nl_pool") if pool else ("CONV2D_TYPE", "conv2d", "forward_conv2d")
            layers.append(dict(name=lname, kind=kind, fields=fields, inp=cur, out=out, params=[wt, bt]))
        elif s[0] == "dense":
            n_in, n_out = cur["n"], s[1]
            view = dict(_hwc(cur["name"] + "0", 1, 1, n_in), array=cur["array"])
            tensors.append(view)
            W = rng.normal(0, 1.0 / np.sqrt(n_in), (n_out, n_in)).astype(np.float32)
            B = rng.normal(0, 0.1, n_out).astype(np.float32)
            wt = add_weights(lname + "_weights", (n_in, n_out, 1, 1), (4, 4, 4 * n_in, 4 * n_in * n_out), W.reshape(-1))
            bt = add_weights(lname + "_bias", (1, n_out, 1, 1), (4, 4, 4 * n_out, 4 * n_out), B)
            out = _hwc(lname + "_output", 1, 1, n_out)
            layers.append(dict(name=lname, kind=("DENSE_TYPE", "dense", "forward_dense"), fields=[], inp=view, out=out, params=[wt, bt]))
        elif s[0] in ("relu", "softmax"):
            out = _hwc(lname + "_output", cur["shape"][3], cur["shape"][2], cur["shape"][1])
            fwd = "forward_relu" if s[0] == "relu" else "forward_sm"
            layers.append(dict(name=lname, kind=("NL_TYPE", "nl", fwd), fields=[], inp=cur, out=out, params=None))
        else:
            raise ValueError(s)
        if lname in overrides:
            layers[-1].update(overrides[lname])
        tensors.append(out)
        arrays[out["array"]] = (out["n"], "AI_ARRAY_FORMAT_FLOAT")
        cur = out

    L = ["/* generated in X-CUBE-AI's format from seeded random weights */", '#include "%s.h"' % name, ""]
    for a, (n, fmt) in arrays.items():
        L.append("AI_ARRAY_OBJ_DECLARE(\n    %s, %s,\n    NULL, NULL, %d,\n     AI_STATIC)" % (a, fmt, n))
    for t in tensors:
        L.append("AI_TENSOR_OBJ_DECLARE(\n  %s, AI_STATIC,\n  0x0, 0x0, AI_SHAPE_INIT(4, %d, %d, %d, %d), AI_STRIDE_INIT(4, %d, %d, %d, %d),\n  1, &%s, NULL)"
                 % ((t["name"],) + tuple(t["shape"]) + tuple(t["stride"]) + (t["array"],)))
    for i, ly in enumerate(layers):
        p = "AI_TENSOR_LIST_ENTRY(%s, NULL)" % ", ".join("&" + x for x in ly["params"]) if ly["params"] else "AI_TENSOR_LIST_EMPTY"
        L.append("AI_TENSOR_CHAIN_OBJ_DECLARE(\n  %s_chain, AI_STATIC_CONST, 4,\n  AI_TENSOR_LIST_ENTRY(&%s),\n  AI_TENSOR_LIST_ENTRY(&%s),\n  %s,\n  AI_TENSOR_LIST_EMPTY\n)"
                 % (ly["name"], ly["inp"]["name"], ly["out"]["name"], p))
        nxt = layers[i + 1]["name"] if i + 1 < len(layers) else ly["name"]
        f = "".join(", \n  %s" % x for x in [".tensors = &%s_chain" % ly["name"]] + ly["fields"])
        L.append("AI_LAYER_OBJ_DECLARE(\n  %s, %d,\n  %s,\n  %s, %s,\n  &AI_NET_OBJ_INSTANCE, &%s, AI_STATIC%s, \n)"
                 % (ly["name"], i, ly["kind"][0], ly["kind"][1], ly["kind"][2], nxt, f))
    L.append("AI_NETWORK_OBJ_DECLARE(\n  AI_NET_OBJ_INSTANCE, AI_STATIC,\n  AI_BUFFER_OBJ_INIT(AI_BUFFER_FORMAT_U8,\n                     1, 1, %d, 1,\n                     NULL),\n"
             "  AI_BUFFER_OBJ_INIT(AI_BUFFER_FORMAT_U8,\n                     1, 1, 0, 1,\n                     NULL),\n"
             "  AI_TENSOR_LIST_IO_ENTRY(AI_FLAG_NONE, AI_NET_IN_NUM, &%s),\n  AI_TENSOR_LIST_IO_ENTRY(AI_FLAG_NONE, AI_NET_OUT_NUM, &%s),\n  &%s, 0, NULL)"
             % (len(blob), t_in["name"], cur["name"], layers[0]["name"]))
    L.append("AI_DECLARE_STATIC\nai_bool %s_configure_weights(\n  ai_network* net_ctx, const ai_buffer* weights_buffer)\n{\n  ai_ptr weights = AI_PTR(weights_buffer->data);\n  {" % name)
    for a, off in woff.items():
        L.append("    %s.data = AI_PTR(weights + %d);\n    %s.data_start = AI_PTR(weights + %d);" % (a, off, a, off))
    L.append("  }\n  return true;\n}\n")
    rows = [", ".join("0x%02x" % b for b in blob[i:i + 10]) for i in range(0, len(blob), 10)]
    data = ('#include "%s_data.h"\n\nai_handle ai_%s_data_weights_get(void)\n{\n  AI_ALIGNED(4)\n  static const ai_u8 s_%s_weights[ %d ] = {\n    %s\n  };\n'
            "  return AI_HANDLE_PTR(s_%s_weights);\n}\n" % (name, name, name, len(blob), ",\n    ".join(rows), name))
    return "\n\n".join(L), data


def import_sources(net_c, data_c):
    """The .ednf blob the importer makes of such sources."""
    return cube_import.build_blob(cube_import.convert(cube_import.parse_net_c(net_c), cube_import.parse_data_c(data_c)))
