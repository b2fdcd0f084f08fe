"""CPU tests of the any-geometry KWS interface (edison_kws_geom, kws.geometry.KwsGeometry): the record the C-ABI takes, its defaults
and the frame arithmetic that decides whether a graph accepts a geometry. The GPU side is tests/test_gpu_kws_geom.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_record_matches_the_header():
    from edison_amd import _lib
    text = open(os.path.join(ROOT, "include", "edison_hip.h")).read()
    body = re.search(r"typedef struct edison_kws_geom \{(.*?)\} edison_kws_geom;", text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip() for n in re.sub(r"^(int32_t|double)\s+", "", decl).split(",")]
    assert names == [f for f, _ in _lib.KwsGeom._fields_]
    assert ctypes.sizeof(_lib.KwsGeom) == 8 * 4 + 5 * 8
    for name in ("edison_kws_geom_default", "edison_kws_geom_batch_dev", "edison_kws_geom_batch"):
        assert name in _lib.SIGNATURES and name + "(" in text


def test_from_config_is_the_shipped_geometry():
    from edison_amd import _lib
    from edison_amd import config as cfg
    from edison_amd.kws.geometry import KwsGeometry
    g = KwsGeometry.from_config()
    assert (g.variant, g.use_log, g.frame_len, g.frame_step, g.n_samples, g.mel_nbins, g.first_mfcc, g.num_mfcc) == \
        (_lib.MFCC_B, False, 1024, 1024, 32000, 32, 0, 13)
    assert (g.sample_rate, g.lower_edge_hertz, g.upper_edge_hertz, g.mel_mtx_scale, g.net_input_scale) == (16000.0, 80.0, 7600.0, 128.0, 1.0)
    assert g.frame_count == cfg.n_frames == _lib.UTT_FRAMES and g.n_features == _lib.NET_IN
    c = g.to_ctypes()
    assert (c.variant, c.frame_count, c.num_mfcc) == (_lib.MFCC_B, 0, 13)
    assert KwsGeometry.from_config(use_log=True).to_ctypes().variant == _lib.MFCC_B | _lib.MFCC_USE_LOG


def test_geometries_of_the_retrained_graphs_fit_their_inputs():
    """frame_count x num_mfcc = in_h x in_w x in_c for the committed alt_models graphs at the geometries the GPU tests run them at."""
    from edison_amd import nnom_import
    from edison_amd.kws.geometry import KwsGeometry
    want = {"kws_small": (512, 1024, 32000, 13, 31), "same_stride": (800, 800, 16000, 12, 20), "square": (480, 240, 15600, 16, 64),
            "even_same": (1000, 500, 8500, 20, 16), "odd_no_softmax": (441, 441, 11907, 7, 27)}
    for name, (n, step, ns, num, frames) in want.items():
        with open(os.path.join(ROOT, "tests", "golden", "alt_models", name + ".h")) as f:
            shape, _ = nnom_import.parse_weights_h(f.read())
        g = KwsGeometry.from_config(frame_len=n, frame_step=step, n_samples=ns, num_mfcc=num)
        assert g.frame_count == frames and g.n_features == shape[0] * shape[1] * shape[2], name
    assert KwsGeometry.from_config(frame_count_=5).frame_count == 5
