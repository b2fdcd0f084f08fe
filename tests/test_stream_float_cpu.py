"""CPU tests of the float-network stream's plumbing (no GPU): the C-ABI declares and the binding exposes edison_stream_float_*, the
library builds the new sources, the two kernels on its hot path use no scratch, and the reference answer the GPU tests build on the host
(test_gpu_stream_float: F - 1 zero rows, then one row per frame, windows oldest first, the network by tests/fnet_host.py) agrees with
the batch form wherever a window is full."""
import os
import re
import subprocess
from dataclasses import replace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["default_opts", "create", "destroy", "reset", "push", "push_dev", "push_n_dev", "frames_seen", "filtered", "filtered_dev", "fsm",
         "fsm_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "edison_hip.h")).read()


def test_header_and_binding_declare_the_stream():
    from edison_amd import _lib
    text = _header()
    declared = set(re.findall(r"\b(edison_stream_float_\w+)\s*\(", text))
    assert declared == {"edison_stream_float_" + n for n in NAMES}
    assert declared <= set(_lib.SIGNATURES)


def test_opts_struct_matches_the_header():
    """StreamFloatOpts._fields_ in the header's order and types."""
    import ctypes
    from edison_amd import _lib
    body = re.search(r"typedef struct edison_stream_float_opts \{(.*?)\} edison_stream_float_opts;", _header(), re.S).group(1)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    ctypes_of = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}
    assert [(f, ctypes_of[t]) for f, t in fields] == [(f, t) for f, t in _lib.StreamFloatOpts._fields_]
    assert [f for f, _ in fields] == ["chunk_frames", "q15", "clip_lo", "clip_hi", "filter", "fsm", "filter_alpha", "true_threshold"]


def _compile(tmp_path, name, extra=()):
    from edison_amd import build as B
    cmd = [B._hipcc(), "--offload-arch=" + B.ARCH, "-std=c++17", "-fno-slp-vectorize", "-O3", "-I" + B.CSRC] + list(extra) + \
        B.PER_FILE_FLAGS.get(name, []) + ["-c", "-x", "hip", os.path.join(B.CSRC, name), "-o", str(tmp_path / (name + ".o"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def test_the_stream_is_built(tmp_path):
    """build.HIP_SOURCES lists the host object, the sliding-window core and the new MFCC instance, and all cross-compile for gfx950 on
    the library's flags."""
    from edison_amd import build
    for name in ("edison_float_bank.hip", "edison_stream_core.hip", "mfcc_geom_fnet_kernels.hip"):
        assert name in build.HIP_SOURCES
        _compile(tmp_path, name, ["-Wall", "-Wextra", "-Wno-unused-parameter", "-fPIC"])
    for h in ("mfcc_geom_device.h", "edison_stream_core.h"):
        assert h in build.HEADERS
        assert os.path.exists(os.path.join(build.CSRC, h))
    assert "edison_stream_kernels.h" not in build.HEADERS


def _scratch(text):
    out = {}
    for b in re.split(r"remark: Function Name: ", text)[1:]:
        out[b.split()[0]] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    return out


def test_hot_path_kernels_use_no_scratch(tmp_path):
    """Both teams of the float network-input MFCC instance and the strided network kernel: no scratch, on the library's flags."""
    seen = _scratch(_compile(tmp_path, "mfcc_geom_fnet_kernels.hip", ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]))
    want = ["_Z24ed_mfcc_geom_fnet_kernelILi64EEv14ed_geom_args_tPffff", "_Z24ed_mfcc_geom_fnet_kernelILi256EEv14ed_geom_args_tPffff"]
    assert sorted(seen) == sorted(want) and all(seen[k] == 0 for k in want), seen
    seen = _scratch(_compile(tmp_path, "fnet_kernels.hip", ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]))
    net = [k for k in seen if "ed_fnet_kernel" in k]
    assert len(net) == 1 and seen[net[0]] == 0, seen
    assert "ll" in net[0].split("ed_fnet_plan_t")[1][:12]   # the input stride (int64) beside the count


def test_one_frame_body_for_the_third_instance():
    """The new instance computes y by the shared frame body and stores the float network input; the filter and shift kernels exist once,
    in the sliding-window core (edison_stream_core.hip): neither front end (one file per network type, stream and bank) defines a kernel,
    and both run their pushes through the core's entry points, begin_push (which shifts) and finish_push (which filters)."""
    from edison_amd import build as B
    kern = open(os.path.join(B.CSRC, "mfcc_geom_fnet_kernels.hip")).read()
    assert kern.count('#include "mfcc_geom_frames.inc"') == 1 and "a.dct_div" not in kern
    assert "fminf(fmaxf((float)(y) * scale, lo), hi)" in kern
    for name in ("edison_float_bank.hip", "edison_stream_bank.hip"):
        text = open(os.path.join(B.CSRC, name)).read()
        assert "__global__" not in text and "hipLaunchKernelGGL" not in text
        assert "ed_stream_core_begin_push(" in text and "ed_stream_core_finish_push(" in text
        # one device push and one host push per network type: the stream API forwards to the bank's and has no push of its own
        assert text.count("ed_stream_core_begin_push(") == 2, name
    core = open(os.path.join(B.CSRC, "edison_stream_core.hip")).read()
    assert core.count("__global__") == 2
    # the filter's arithmetic and its one no-contraction pragma live in the shared header, not here
    assert core.count("#pragma clang fp contract(off)") == 0
    assert open(os.path.join(B.CSRC, "edison_postproc_core.h")).read().count("#pragma clang fp contract(off)") == 1
    assert core.count("void ed_stream_core_shift_kernel(") == 1 and core.count("void ed_stream_core_filter_kernel(") == 1
    assert "ed_stream_core_filter_kernel<int8_t>" in core and "ed_stream_core_filter_kernel<float>" in core
    # the shift is launched in one place, make_room, which begin_push calls; the filter in one place, launch_filter, which both finish
    # functions call
    assert core.count("hipLaunchKernelGGL(ed_stream_core_shift_kernel") == 1 and core.count("hipLaunchKernelGGL(ed_stream_core_filter_kernel<") == 2
    assert core.count("hipLaunchKernelGGL(") == 3
    room = core[core.index("static int make_room("):core.index("int ed_stream_core_check_opts(")]
    assert "hipLaunchKernelGGL(ed_stream_core_shift_kernel" in room
    begin = core[core.index("int ed_stream_core_begin_push("):core.index("static int launch_filter(")]
    assert "make_room(c, q, n)" in begin
    helper = core[core.index("static int launch_filter("):core.index("static int end_push(")]
    assert helper.count("hipLaunchKernelGGL(ed_stream_core_filter_kernel<") == 2
    plain = core[core.index("int ed_stream_core_finish_push("):core.index("int ed_stream_core_finish_push_present(")]
    masked = core[core.index("int ed_stream_core_finish_push_present("):core.index("int ed_stream_core_frames_seen_mics(")]
    assert "launch_filter(c, q, NULL, fin, n)" in plain and "launch_filter(c, q, present, fin, n)" in masked
    # nothing the core provides is defined a second time anywhere in the library's sources
    texts = [open(os.path.join(B.CSRC, f)).read() for f in sorted(os.listdir(B.CSRC)) if f.endswith((".hip", ".h", ".c", ".inc"))]
    for fn in ("order_after", "make_room", "copy_out", "ed_stream_core_filtered", "ed_stream_core_fsm", "ed_stream_core_reset",
               "ed_stream_core_free", "launch_filter"):
        assert sum(len(re.findall(r"^(?:static )?(?:int|void) %s\(.*\)\n\{" % fn, x, re.M)) for x in texts) == 1, fn
    for kernel in ("ed_stream_core_shift_kernel", "ed_stream_core_filter_kernel"):
        assert sum(len(re.findall(r"\bvoid %s\(" % kernel, x)) for x in texts) == 1, kernel


def _float_rows(oracle_mod, g, z, starts):
    """float32 [n][F * num_mfcc]: the host flow's network input of the utterances of z at `starts` (oracle MFCC, float32 x scale, clip)."""
    import geom_sweep
    y = geom_sweep.oracle_mfcc(oracle_mod, z, g, starts)
    return np.clip(y.astype(np.float32) * np.float32(g.net_input_scale), np.float32(-32768), np.float32(32767)).reshape(len(starts), -1)


@pytest.mark.parametrize("name", ["kws_small", "square", "odd_no_softmax"])
def test_host_reference_agrees_with_the_batch_form(oracle_mod, name):
    """The GPU tests' reference: one row per frame of the zero-led recording, F - 1 zero rows in front, windows oldest first, the network
    by fnet_host. For k >= F - 1 window k is the batch form's features of the utterance at (k - F + 1) * frame_step, and the exact model
    gives the same logits on it; window 0 is F - 1 zero rows and frame 0's row."""
    import cube_synth
    import fnet_host
    from edison_amd import cube_import
    from geom_sweep import GEOMS, geom
    from stream_drive import SYNTH, import_sources, recording, tail
    g = geom(**GEOMS[name])
    F, nm = g.frame_count, g.num_mfcc
    K = F + 5
    x = recording(g, K, 3)
    z = np.concatenate([np.zeros(tail(g), np.int16), x])
    # one row per frame: frame k is the MFCC of z[k * frame_step ..)
    one = replace(g, frame_count_=1, n_samples=g.frame_len)
    rows = np.stack([_float_rows(oracle_mod, one, z, [k * g.frame_step])[0] for k in range(K)])
    r = np.concatenate([np.zeros((F - 1, nm), np.float32), rows])
    win = np.stack([r[k:k + F].reshape(-1) for k in range(K)])
    batch = _float_rows(oracle_mod, g, z, [(k - F + 1) * g.frame_step for k in range(F - 1, K)])
    assert np.array_equal(win[F - 1:], batch)
    assert not win[0, :(F - 1) * nm].any() and np.array_equal(win[0, (F - 1) * nm:], rows[0])
    model = cube_import.read_blob(import_sources(cube_synth.cube_sources((F, nm, 1), SYNTH, seed=len(name))))
    assert np.array_equal(fnet_host.run(model, win[F - 1:])[-1], fnet_host.run(model, batch)[-1])
