"""The MFCC geometry a keyword-spotting graph was trained at -- the values the reference's training flow reads from ``audio/config.py``
(frame_length, frame_step, num_mel_bins, first_mfcc / num_mfcc, the mel edges, net_input_scale; kws_keras.py:443-468) -- as the
``edison_kws_geom`` record of the C-ABI (include/edison_hip.h, ``edison_kws_geom_batch*``). ``Context.kws_geom`` runs audio to class
index at such a geometry in one call; the features, logits and argmax are the reference host flow's (float64 MFCC)."""
from dataclasses import dataclass, replace

from .. import _lib
from .. import config as cfg


@dataclass(frozen=True)
class KwsGeometry:
    variant: int = _lib.MFCC_B          # _lib.MFCC_A or _lib.MFCC_B (mfcc / mfcc_mcu)
    use_log: bool = False               # variant B only: mfcc_mcu(..., use_log=True)
    frame_len: int = cfg.frame_length
    frame_step: int = cfg.frame_length
    n_samples: int = cfg.nSamples       # one utterance
    frame_count_: int = 0               # 0: as many frames as fit (audio/config.py's frame_count)
    mel_nbins: int = cfg.num_mel_bins
    first_mfcc: int = cfg.first_mfcc
    num_mfcc: int = cfg.num_mfcc
    sample_rate: float = float(cfg.fs)
    lower_edge_hertz: float = cfg.lower_edge_hertz
    upper_edge_hertz: float = cfg.upper_edge_hertz
    mel_mtx_scale: float = float(cfg.mel_mtx_scale)
    net_input_scale: float = cfg.nnom_net_input_scale

    @classmethod
    def from_config(cls, **changes):
        """audio/config.py's geometry (variant B, 1024 / 1024, 32000 samples, 32 mel bins, first 13 coefficients), with `changes`."""
        return replace(cls(), **changes)

    @property
    def frame_count(self):
        if self.frame_count_:
            return self.frame_count_
        return 1 + (self.n_samples - self.frame_len) // self.frame_step if self.n_samples >= self.frame_len else 0

    @property
    def n_features(self):
        """int8 features per utterance: frame_count x num_mfcc (must equal the graph's in_h x in_w x in_c)."""
        return self.frame_count * self.num_mfcc

    def to_ctypes(self):
        g = _lib.KwsGeom()
        g.variant = int(self.variant) | (_lib.MFCC_USE_LOG if self.use_log else 0)
        g.frame_len, g.frame_step, g.n_samples, g.frame_count = int(self.frame_len), int(self.frame_step), int(self.n_samples), int(self.frame_count_)
        g.mel_nbins, g.first_mfcc, g.num_mfcc = int(self.mel_nbins), int(self.first_mfcc), int(self.num_mfcc)
        g.sample_rate, g.lower_edge_hertz, g.upper_edge_hertz = float(self.sample_rate), float(self.lower_edge_hertz), float(self.upper_edge_hertz)
        g.mel_mtx_scale, g.net_input_scale = float(self.mel_mtx_scale), float(self.net_input_scale)
        return g
