"""CPU tests of float64 MFCC at any geometry (no GPU): the C-ABI and the binding declare edison_mfcc_geom_batch* alike, the float64
instances of the any-geometry kernel are built without scratch, and dataset_features(..., geometry=) refuses what it must before it
touches a device. The GPU side is tests/test_gpu_mfcc_geom.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("edison_mfcc_geom_batch_dev", "edison_mfcc_geom_batch")
# C parameter type -> the ctypes type _lib declares for it
CTYPES = {"edison_ctx *": ctypes.c_void_p, "const int16_t *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "double *": ctypes.c_void_p}


def test_header_and_binding_declare_both_forms_alike():
    from edison_amd import _lib
    text = open(os.path.join(ROOT, "include", "edison_hip.h")).read()
    for name in NAMES:
        m = re.search(r"\bint %s\((.*?)\);" % name, text, flags=re.S)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).split(",")]
        types = [re.match(r"(.*?[\s*])\w+$", p).group(1).strip() for p in params]
        types = [re.sub(r"\s*\*", " *", t) for t in types]
        assert types == ["edison_ctx *", "const edison_kws_geom *", "const int16_t *", "int64_t", "int64_t", "double *"], (name, types)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(types), name
        for t, a in zip(types, args):
            want = ctypes.POINTER(_lib.KwsGeom) if t == "const edison_kws_geom *" else CTYPES[t]
            assert a is want, (name, t, a)


def test_float64_instances_use_no_scratch(tmp_path):
    """Both teams of ed_mfcc_geom_f64_kernel exist beside the int8 instances, on the library's build flags, and none spills."""
    from edison_amd import build as B
    cmd = [B._hipcc(), "--offload-arch=" + B.ARCH, "--cuda-device-only", "-c", "-std=c++17", "-fno-slp-vectorize", "-O3", "-I" + B.CSRC,
           "-Rpass-analysis=kernel-resource-usage", "-x", "hip", os.path.join(B.CSRC, "mfcc_geom_kernels.hip"), "-o", str(tmp_path / "g.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        seen[name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    want = ["_Z19ed_mfcc_geom_kernelILi64EEv14ed_geom_args_t", "_Z19ed_mfcc_geom_kernelILi256EEv14ed_geom_args_t",
            "_Z23ed_mfcc_geom_f64_kernelILi64EEv14ed_geom_args_tPd", "_Z23ed_mfcc_geom_f64_kernelILi256EEv14ed_geom_args_tPd"]
    for k in want:
        assert seen.get(k) == 0, (k, seen)


def test_one_body_computes_y_for_every_instance():
    """Stage 6's y is computed once, in the shared body; each kernel only says what it stores."""
    from edison_amd import build as B
    body = open(os.path.join(B.CSRC, "mfcc_geom_frames.inc")).read()
    kern = open(os.path.join(B.CSRC, "mfcc_geom_kernels.hip")).read()
    assert "y = y / a.dct_div;" in body and "EDG_STORE(" in body
    assert "a.dct_div" not in kern and kern.count('#include "mfcc_geom_frames.inc"') == 2
    assert "mfcc_geom_frames.inc" in B.HEADERS


class _NoDevice:
    """A context that fails the test when anything is asked of it."""

    def __getattr__(self, name):
        raise AssertionError("dataset_features touched the device (%s)" % name)


@pytest.mark.parametrize("kw", [dict(fs=8000), dict(nSamples=16000), dict(frame_length=512), dict(frame_step=512), dict(frame_count=10),
                                dict(num_mel_bins=40), dict(lower_edge_hertz=20.0), dict(upper_edge_hertz=4000.0), dict(mel_mtx_scale=64),
                                dict(use_mfcc_log=True), dict(first_mfcc=1), dict(num_mfcc=12), dict(net_input_scale=0.5)])
def test_dataset_features_refuses_geometry_keywords_beside_a_geometry(kw):
    from edison_amd.kws.features import dataset_features
    from edison_amd.kws.geometry import KwsGeometry
    with pytest.raises(ValueError, match=list(kw)[0]):
        dataset_features(np.zeros((2, 32000), np.int16), geometry=KwsGeometry.from_config(), ctx=_NoDevice(), **kw)


def test_dataset_features_with_a_geometry_checks_before_the_device():
    from edison_amd import config as cfg
    from edison_amd.kws.features import dataset_features
    from edison_amd.kws.geometry import KwsGeometry
    g = KwsGeometry.from_config(frame_len=400, frame_step=160, n_samples=16000, mel_nbins=40, num_mfcc=13)
    with pytest.raises(ValueError, match="shorter"):
        dataset_features(np.zeros((3, 15999), np.int16), geometry=g, ctx=_NoDevice())
    # the defaults, given explicitly, and the clip bounds are not geometry keywords
    e = dataset_features(np.zeros((0, 16000), np.int16), geometry=g, ctx=_NoDevice(), fs=cfg.fs, num_mfcc=cfg.num_mfcc,
                         net_input_clip_min=-100, net_input_clip_max=100)
    assert e.shape == (0, 98, 13, 1) and e.dtype == np.float64
