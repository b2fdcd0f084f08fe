"""CPU tests of the float bank's plumbing (no GPU): the C-ABI declares and the binding exposes edison_float_bank_*, the library builds
the bank's sources, the two-stride network kernel and both instances of the banked filter use no scratch, the network kernel keeps f32
subnormals and runs on the f32 matrix cores, and the calls that need no device answer as the header says."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["default_opts", "create", "destroy", "reset", "reset_mic", "push", "push_dev", "push_n_dev", "filtered", "filtered_dev", "fsm", "fsm_dev",
         "frames_seen"]


def _compile(tmp_path, name, extra=()):
    """One source for gfx950 on the library's flags; returns the compiler's stderr."""
    from edison_amd import build as B
    cmd = [B._hipcc(), "--offload-arch=" + B.ARCH, "-std=c++17", "-fno-slp-vectorize", "-O3", "-I" + B.CSRC] + list(extra) + \
        B.PER_FILE_FLAGS.get(name, []) + ["-x", "hip", os.path.join(B.CSRC, name), "-o", str(tmp_path / (name + ".out"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _scratch(text):
    out = {}
    for b in re.split(r"remark: Function Name: ", text)[1:]:
        out[b.split()[0]] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    return out


def test_header_and_binding_declare_the_bank():
    from edison_amd import _lib
    text = open(os.path.join(ROOT, "include", "edison_hip.h")).read()
    declared = set(re.findall(r"\b(edison_float_bank_\w+)\s*\(", text))
    assert len(NAMES) == 13 and declared == {"edison_float_bank_" + n for n in NAMES}
    assert declared <= set(_lib.SIGNATURES)
    assert {k for k in _lib.SIGNATURES if k.startswith("edison_float_bank_")} == declared
    L = _lib.lib()
    for name in declared:
        assert getattr(L, name)


def test_opts_layout():
    from edison_amd import _lib
    assert [f for f, _ in _lib.FloatBankOpts._fields_] == ["n_mics", "stream"]
    assert _lib.FloatBankOpts._fields_[1][1] is _lib.StreamFloatOpts
    assert _lib.FloatBankOpts.stream.offset == 8 and ctypes.sizeof(_lib.FloatBankOpts) == 8 + ctypes.sizeof(_lib.StreamFloatOpts)


def test_the_bank_is_built(tmp_path):
    """build.HIP_SOURCES / HEADERS list the bank's host object, the two-stride network kernel and the shared device header, and the new
    and changed sources cross-compile for gfx950 with -Wall -Wextra."""
    from edison_amd import build
    for name in ("edison_float_bank.hip", "fnet_windows_kernels.hip", "fnet_kernels.hip"):
        assert name in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC, name))
        err = _compile(tmp_path, name, ["-Wall", "-Wextra", "-Wno-unused-parameter", "-fPIC", "-c"])
        assert not [ln for ln in err.splitlines() if "warning:" in ln and "loop not unrolled" not in ln and "argument unused" not in ln], err[-2000:]
    assert "fnet_device.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "fnet_device.h"))
    bank = open(os.path.join(build.CSRC, "edison_float_bank.hip")).read()
    # a host object on the sliding-window core: no kernel of its own
    assert "__global__" not in bank and "hipLaunchKernelGGL" not in bank
    for call in ("ed_stream_core_begin_push(", "ed_stream_core_finish_push(", "ed_stream_core_reset_mic(", "ed_launch_fnet_windows(", "ed_launch_fnet(",
                 "ed_launch_mfcc_geom_fnet(", "ed_ctx_mfcc_q15_launch_on("):
        assert call in bank, call
    # the body of the network kernels exists once, in the header
    for name in ("fnet_kernels.hip", "fnet_windows_kernels.hip"):
        text = open(os.path.join(build.CSRC, name)).read()
        assert '#include "fnet_device.h"' in text and "mfma" not in text.split("*/", 1)[1]


def test_the_window_kernel_uses_no_scratch_and_keeps_subnormals(tmp_path):
    err = _compile(tmp_path, "fnet_windows_kernels.hip", ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"])
    seen = _scratch(err)
    assert len(seen) == 1 and "ed_fnet_windows_kernel" in list(seen)[0] and list(seen.values()) == [0], seen
    asm = (tmp_path / "fnet_windows_kernels.hip.out").read_text()
    assert "v_mfma_f32_16x16x4_f32" in asm or "v_mfma_f32_16x16x4f32" in asm
    assert re.findall(r"\.amdhsa_float_denorm_mode_32 (\d+)", asm) == ["3"]


def test_both_banked_filters_use_no_scratch(tmp_path):
    """The core's kernels, which serve every stream and bank, masked pushes included: the shift and the filter's int8 and float instances."""
    seen = _scratch(_compile(tmp_path, "edison_stream_core.hip", ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]))
    filt = sorted(k for k in seen if "ed_stream_core_filter_kernel" in k)
    assert len(filt) == 2 and filt[0].split("ed_stream_core_filter_kernel")[1][:2] == "Ia" and filt[1].split("ed_stream_core_filter_kernel")[1][:2] == "If", seen
    assert len([k for k in seen if "ed_stream_core_shift_kernel" in k]) == 1
    assert len(seen) == 3 and all(v == 0 for v in seen.values()), seen


def test_calls_that_need_no_device():
    from edison_amd import _lib
    L = _lib.lib()
    o = _lib.FloatBankOpts()
    L.edison_float_bank_default_opts(ctypes.byref(o))
    s = o.stream
    assert (o.n_mics, s.chunk_frames, s.q15, s.clip_lo, s.clip_hi, s.filter, s.fsm, s.filter_alpha, s.true_threshold) == \
        (1, 1, 0, -32768.0, 32767.0, 0, 0, 0.5, 0.5)
    L.edison_float_bank_default_opts(None)
    L.edison_float_bank_destroy(None)
    n = ctypes.c_int64(7)
    assert L.edison_float_bank_reset(None) == _lib.E_ARGUMENT and L.edison_float_bank_reset_mic(None, 0) == _lib.E_ARGUMENT
    assert L.edison_float_bank_frames_seen(None, ctypes.byref(n)) == _lib.E_ARGUMENT and n.value == 7
    assert L.edison_float_bank_create(None, None, None, None) == _lib.E_ARGUMENT
    for r in (L.edison_float_bank_push(None, None, None, None, None), L.edison_float_bank_push_dev(None, None, None, None, None),
              L.edison_float_bank_push_n_dev(None, None, 1, None, None, None), L.edison_float_bank_filtered(None, None, None, None),
              L.edison_float_bank_filtered_dev(None, None, None, None), L.edison_float_bank_fsm(None, None, None),
              L.edison_float_bank_fsm_dev(None, None, None)):
        assert r == _lib.E_ARGUMENT
