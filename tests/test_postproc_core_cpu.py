"""CPU tests (no GPU) of the output filter's one home, edison_postproc_core.h: the no-contraction pragma and the two operations it guards
exist once in the library's sources, every kernel that filters steps through them, and the device code of those kernels rounds the
product and the sum separately -- double multiplies and adds, no fused multiply-add."""
import os
import re
import subprocess

import pytest

PRAGMA = "#pragma clang fp contract(off)"
HEADER = "edison_postproc_core.h"
SITES = ["edison_stream_core.hip", "edison_stream.hip", "cnn_mfma_kernels.hip"]


def _texts():
    from edison_amd import build as B
    return {f: open(os.path.join(B.CSRC, f)).read() for f in sorted(os.listdir(B.CSRC)) if f.endswith((".hip", ".h", ".c", ".inc"))}


def test_the_pragma_exists_once_in_the_shared_header():
    from edison_amd import build as B
    assert HEADER in B.HEADERS
    assert {f: x.count(PRAGMA) for f, x in _texts().items() if PRAGMA in x} == {HEADER: 1}
    # the header the run-time compiler embeds does not pull it in
    assert HEADER not in _texts()["edison_internal.h"]


def test_the_two_operations_are_defined_once_and_every_site_steps_through_them():
    texts = _texts()
    for fn, ret in (("ed_filter_term", "double"), ("ed_filter_step", "float")):
        where = {f: len(re.findall(r"^ED_PP_FN %s %s\(" % (ret, fn), x, re.M)) for f, x in texts.items()}
        assert {f: n for f, n in where.items() if n} == {HEADER: 1}, fn
    head = texts[HEADER]
    # both sit under the pragma: behind it, before contraction is handed back
    guarded = head[head.index(PRAGMA):head.index("#pragma clang fp contract(fast)")]
    assert "ed_filter_term(" in guarded and "ed_filter_step(" in guarded
    for name in SITES:
        assert "ed_filter_step(" in texts[name] and "ed_filter_term(" in texts[name], name
    # the one state-machine stage struct
    assert sum(len(re.findall(r"^struct ed_fsm_stage_t\b", x, re.M)) for x in texts.values()) == 1 and "struct ed_fsm_stage_t" in head
    assert not any("edsg_fsm_stage_t" in x for x in texts.values())


def test_the_build_refuses_another_contraction_setting(monkeypatch):
    """The header hands contraction back as contract(fast), hipcc's own setting: a product build may not ask for another."""
    from edison_amd import build as B
    monkeypatch.setenv("ED_CFLAGS", "-g")
    assert B.product_flags() == ["-g"]
    for flag in ("-ffp-contract=off", "-ffp-contract=on"):
        monkeypatch.setenv("ED_CFLAGS", "-g " + flag)
        with pytest.raises(RuntimeError, match="ffp-contract"):
            B.product_flags()


@pytest.mark.parametrize("name", SITES)
def test_the_device_code_rounds_product_and_sum_separately(tmp_path, name):
    from edison_amd import build as B
    out = tmp_path / (name + ".s")
    cmd = [B._hipcc(), "--offload-arch=" + B.ARCH, "-std=c++17", "-fno-slp-vectorize", "-O3", "-fPIC", "-I" + B.CSRC] + B.PER_FILE_FLAGS.get(name, []) + \
        ["--cuda-device-only", "-S", "-x", "hip", os.path.join(B.CSRC, name), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    assert "v_fma_f64" not in asm and "v_fmac_f64" not in asm
