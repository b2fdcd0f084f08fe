"""CPU tests (no GPU) of bank pushes that leave microphones out: the C-ABI declares and the binding exposes the six entry points, the
library builds and exports them, the hold's source cross-compiles for gfx950 without warnings and its kernel uses no scratch, the calls that
need no device answer as the header says, and the hold kernel's rounds -- restated in numpy -- equal a memmove on rows whose source and
destination overlap and on rows where they do not, where ascending rounds go wrong on exactly the former."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "edison_bank_hold.hip"
NAMES = ["push_present", "push_present_n_dev", "frames_seen_mics"]
NEW = ["edison_bank_" + n for n in NAMES] + ["edison_fbank_" + n for n in NAMES]


def test_header_and_binding_declare_the_entry_points(built_lib):
    from edison_amd import _lib
    text = open(os.path.join(ROOT, "include", "edison_hip.h")).read()
    declared = set(re.findall(r"\b(edison_f?bank_\w+)\s*\(", text))
    assert declared == set(NEW)
    assert {k for k in _lib.SIGNATURES if re.match(r"edison_f?bank_", k)} == declared
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name)
    # the same arguments for both banks: the push's, with the mask behind the samples
    for n in NAMES:
        assert _lib.SIGNATURES["edison_bank_" + n] == _lib.SIGNATURES["edison_fbank_" + n]
    assert len(_lib.SIGNATURES["edison_bank_push_present"][1]) == len(_lib.SIGNATURES["edison_stream_bank_push"][1]) + 1
    assert len(_lib.SIGNATURES["edison_bank_push_present_n_dev"][1]) == len(_lib.SIGNATURES["edison_stream_bank_push_n_dev"][1]) + 1


def test_python_pushes_take_a_mask():
    import inspect
    from edison_amd.stream import FloatBank, StreamBank
    for cls in (StreamBank, FloatBank):
        for fn in (cls.push, cls.push_t):
            assert inspect.signature(fn).parameters["present"].default is None
        assert callable(cls.frames_seen_mics)


def _compile(tmp_path, extra):
    """The new source for gfx950 on the library's flags; returns the compiler's stderr."""
    from edison_amd import build as B
    cmd = [B._hipcc(), "--offload-arch=" + B.ARCH, "-std=c++17", "-fno-slp-vectorize", "-O3", "-I" + B.CSRC] + list(extra) + \
        B.PER_FILE_FLAGS.get(SOURCE, []) + ["-x", "hip", os.path.join(B.CSRC, SOURCE), "-o", str(tmp_path / (SOURCE + ".out"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def test_the_source_is_built_without_warnings(tmp_path):
    """build.HIP_SOURCES lists the file; it holds one kernel, the hold, and its launcher -- the masked filter is the core's filter kernel
    given the mask, so no filter arithmetic and no pragma here -- and cross-compiles for gfx950 with -Wall -Wextra."""
    from edison_amd import build
    assert SOURCE in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC, SOURCE))
    err = _compile(tmp_path, ["-Wall", "-Wextra", "-Wno-unused-parameter", "-fPIC", "-c"])
    assert not [ln for ln in err.splitlines() if "warning:" in ln and "argument unused" not in ln], err[-2000:]
    text = open(os.path.join(build.CSRC, SOURCE)).read()
    assert text.count("__global__") == 1 and "#pragma clang fp contract" not in text
    assert "void ed_bank_launch_hold(" in text
    texts = [open(os.path.join(build.CSRC, f)).read() for f in sorted(os.listdir(build.CSRC)) if f.endswith((".hip", ".h", ".c", ".inc"))]
    assert not any("ed_bank_launch_filter_present" in x for x in texts)
    core = open(os.path.join(build.CSRC, "edison_stream_core.hip")).read()
    masked = core[core.index("int ed_stream_core_finish_push_present("):core.index("int ed_stream_core_frames_seen_mics(")]
    # the hold, then the shared filter launch with the mask
    assert 0 < masked.index("ed_bank_launch_hold(") < masked.index("launch_filter(c, q, present, fin, n)")


def test_the_hold_kernel_uses_no_scratch(tmp_path):
    """The masked filter's scratch: test_float_bank_cpu.py::test_both_banked_filters_use_no_scratch, on the core's kernels."""
    err = _compile(tmp_path, ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"])
    seen = {}
    for b in re.split(r"remark: Function Name: ", err)[1:]:
        seen[b.split()[0]] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    assert len([k for k in seen if "ed_bank_hold_kernel" in k]) == 1
    assert len(seen) == 1 and all(v == 0 for v in seen.values()), seen


def test_calls_that_need_no_device(built_lib):
    from edison_amd import _lib
    L = _lib.lib()
    x = np.zeros(16, np.int16)
    p = np.ones(1, np.uint8)
    counts = np.full(2, 7, np.int64)
    for pre in ("edison_bank_", "edison_fbank_"):
        assert getattr(L, pre + "push_present")(None, x.ctypes.data, p.ctypes.data, None, None, None) == _lib.E_ARGUMENT
        assert getattr(L, pre + "push_present")(None, None, None, None, None, None) == _lib.E_ARGUMENT
        assert getattr(L, pre + "push_present_n_dev")(None, x.ctypes.data, p.ctypes.data, 1, None, None, None) == _lib.E_ARGUMENT
        assert getattr(L, pre + "frames_seen_mics")(None, counts.ctypes.data) == _lib.E_ARGUMENT
    assert list(counts) == [7, 7]


# ---- the hold's rounds -----------------------------------------------------------------------------------------------------------
def hold_rounds(buf, src, count, by):
    """hold_up of edison_bank_hold.hip: rounds of 256 from the top down; in a round every lane reads, the workgroup waits, every lane
    writes."""
    for top in range(count, 0, -256):
        lo = max(top - 256, 0)
        v = buf[src + lo:src + top].copy()
        buf[src + by + lo:src + by + top] = v


def hold_ascending(buf, src, count, by):
    """The shift kernel's order, which is right for a destination BELOW the source: the same rounds from the bottom up."""
    for base in range(0, count, 256):
        hi = min(base + 256, count)
        v = buf[src + base:src + hi].copy()
        buf[src + by + base:src + by + hi] = v


def _rows():
    """(name, count, by): what the hold moves in the geometries the GPU tests run, for pushes of 1 .. 3 frames -- T history samples up by
    n * hop samples, (F - 1) * nm * elem bytes of rows up by n * nm * elem bytes (elem 1: int8 rows, 4: float32 rows)."""
    geoms = {"shipped": (1024, 1024, 31, 13), "even_same": (1000, 500, 16, 20), "long": (960, 240, 64, 16), "square": (480, 240, 64, 16)}
    out = []
    for name, (frame_len, hop, F, nm) in geoms.items():
        T = max(0, frame_len - hop)
        for n in (1, 2, 3):
            out.append(("%s samples n=%d" % (name, n), T, n * hop))
            for elem in (1, 4):
                out.append(("%s rows x%d n=%d" % (name, elem, n), (F - 1) * nm * elem, n * nm * elem))
    # rows that do not overlap: a push longer than the history
    out += [("short history samples", 300, 4096), ("short history rows", 2 * 13 * 4, 3 * 13 * 4), ("two rounds apart", 512, 512)]
    return out


ROWS = _rows()


def _buffer(count, by, src=37):
    """Distinct tokens: the history at src, poison where the push wrote garbage behind it."""
    buf = -np.arange(1, src + by + count + 64, dtype=np.int64)
    buf[src:src + count] = 1000 + np.arange(count)
    return buf, src


@pytest.mark.parametrize("name,count,by", ROWS, ids=[r[0] for r in ROWS])
def test_the_rounds_equal_a_memmove(name, count, by):
    buf, src = _buffer(count, by)
    want = buf.copy()
    want[src + by:src + by + count] = buf[src:src + count]          # memmove
    hold_rounds(buf, src, count, by)
    assert np.array_equal(buf, want)                                 # the history where the next push looks for it; nothing else touched
    assert np.array_equal(buf[:src], want[:src]) and np.array_equal(buf[src + by + count:], want[src + by + count:])


@pytest.mark.parametrize("name,count,by", ROWS, ids=[r[0] for r in ROWS])
def test_ascending_rounds_go_wrong_on_exactly_the_overlap_rows(name, count, by):
    """Source and destination overlap when by < count. An ascending round then writes over elements by .. by + 255, which a later round
    still has to read as soon as there is one (count > 256): the rounds must run from the top down. Within one round the order does not
    matter (all lanes read before any writes)."""
    buf, src = _buffer(count, by)
    want = buf.copy()
    want[src + by:src + by + count] = buf[src:src + count]
    hold_ascending(buf, src, count, by)
    overlap = 0 < count and by < count
    assert (not np.array_equal(buf, want)) == (overlap and count > 256), (name, count, by)


def test_the_rows_cover_both_buffers_with_and_without_overlap():
    kinds = {(("samples" in n), by < count, count > 256) for n, count, by in ROWS if count}
    for samples in (True, False):
        assert (samples, True, True) in kinds and any(k[0] == samples and not k[1] for k in kinds)
    assert any(count == 0 for _, count, _ in ROWS)                   # tail = 0: nothing to hold
    # T = 720 at n = 1: three rounds, overlapping
    assert ("long samples n=1", 720, 240) in ROWS
    text = open(os.path.join(ROOT, "edison_amd", "csrc", SOURCE)).read()
    assert "for (int top = count; top > 0; top -= 256)" in text and text.count("hold_up(") == 3
