"""CPU tests of the stream bank's plumbing (no GPU): the C-ABI declares and the binding exposes edison_stream_bank_*, the bank is
built, calls that need no device answer as the header says, and the host-only arithmetic of the sliding-window core with several
microphones -- the size of one microphone's buffers -- holds what a push sequence needs, checked from first principles."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["default_opts", "create", "destroy", "reset", "reset_mic", "push", "push_dev", "push_n_dev", "filtered", "filtered_dev", "fsm", "fsm_dev",
         "frames_seen"]


def test_header_and_binding_declare_the_bank():
    from edison_amd import _lib
    text = open(os.path.join(ROOT, "include", "edison_hip.h")).read()
    declared = set(re.findall(r"\b(edison_stream_bank_\w+)\s*\(", text))
    assert declared == {"edison_stream_bank_" + n for n in NAMES}
    assert declared <= set(_lib.SIGNATURES)
    assert [f for f, _ in _lib.StreamBankOpts._fields_] == ["n_mics", "stream"]
    assert _lib.StreamBankOpts.stream.offset == 8 and ctypes.sizeof(_lib.StreamBankOpts) == 8 + ctypes.sizeof(_lib.StreamGeomOpts)


def test_the_bank_is_built_and_is_a_host_object_with_no_kernel():
    from edison_amd import build
    assert "edison_stream_bank.hip" in build.HIP_SOURCES
    # what the stream and the bank once shared through a header are statics of the one file now
    assert "edison_stream_geom.h" not in build.HEADERS and not os.path.exists(os.path.join(build.CSRC, "edison_stream_geom.h"))
    bank = open(os.path.join(build.CSRC, "edison_stream_bank.hip")).read()
    # as the float bank: its shift and filter are the sliding-window core's, reached through begin_push and finish_push
    assert "__global__" not in bank and "hipLaunchKernelGGL" not in bank and "#pragma clang fp contract" not in bank
    assert "ed_stream_core_begin_push(" in bank and "ed_stream_core_finish_push(" in bank and "ed_stream_core_reset_mic(" in bank
    # the network runs on the launchers the single stream uses: no network kernel of the bank's own
    assert "ed_stream_geom_net_on(" in bank and "hipMemcpy" not in bank


def test_calls_that_need_no_device():
    from edison_amd import _lib
    L = _lib.lib()
    o = _lib.StreamBankOpts()
    L.edison_stream_bank_default_opts(ctypes.byref(o))
    assert (o.n_mics, o.stream.chunk_frames, o.stream.filter, o.stream.fsm, o.stream.filter_alpha, o.stream.true_threshold) == (1, 1, 0, 0, 0.9, 0.5)
    L.edison_stream_bank_default_opts(None)
    L.edison_stream_bank_destroy(None)
    n = ctypes.c_int64(7)
    assert L.edison_stream_bank_reset(None) == _lib.E_ARGUMENT and L.edison_stream_bank_reset_mic(None, 0) == _lib.E_ARGUMENT
    assert L.edison_stream_bank_frames_seen(None, ctypes.byref(n)) == _lib.E_ARGUMENT and n.value == 7
    assert L.edison_stream_bank_create(None, None, None, None) == _lib.E_ARGUMENT


PROBE = r"""
#include <stdio.h>
#include "edison_stream_core.h"
int main(void)
{
	const int cases[][6] = {{0, 8, 1, 1024, 31, 13}, {240, 8, 3, 240, 64, 16}, {4095, 1, 7, 1, 2, 1}, {0, 8, 512, 441, 27, 7}};
	for (unsigned i = 0; i < sizeof(cases) / sizeof(cases[0]); i++)
	{
		const int *k = cases[i];
		printf("%d %d %d %d %d %d %zu %zu %zu\n", k[0], k[1], k[2], k[3], k[4], k[5], ed_stream_core_mic_audio(k[0], k[1], k[2], k[3]),
		       ed_stream_core_mic_feat(1, k[4], k[1], k[2], k[5]), ed_stream_core_mic_feat(4, k[4], k[1], k[2], k[5]));
	}
	return 0;
}
"""


def test_one_microphones_buffers_hold_every_push_before_the_shift(tmp_path):
    """pos runs from 0 to slots * chunk frames before the history moves back to the front. Until then the newest frame's samples end at
    tail + pos * hop and the newest window's rows at F - 1 + pos: a microphone's buffers hold exactly that much, so microphone m + 1's
    begin where microphone m's last push can end and no earlier."""
    from edison_amd import build as B
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    rocm = os.path.dirname(os.path.dirname(B._hipcc()))
    r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + B.CSRC, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"),
                        str(src), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([B._hipcc(), "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + B.CSRC, "-I" + os.path.join(ROOT, "include"), str(src),
                            "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(lines) == 4
    for ln in lines:
        tail, slots, chunk, hop, F, nm, audio, feat1, feat4 = (int(v) for v in ln.split())
        last = slots * chunk                              # frames behind the history when the buffers are full
        assert audio == tail + last * hop                 # the samples of the last frame end here
        assert feat1 == (F - 1 + last) * nm and feat4 == 4 * feat1
        # every push sequence that make_room lets through stays inside: pos + n <= slots * chunk
        for pos in (0, last - chunk, last - 1):
            for n in (1, chunk):
                if pos + n <= last:
                    assert tail + (pos + n) * hop <= audio and (F - 1 + pos + n) * nm <= feat1
