"""tests/fcal_ref.py for padded float networks: the calibration statistic on fnet_pad's bit-exact model. Test
infrastructure, not a test.

The convention is fcal_ref's: for a record v = acc + bias in f32, before ReLU and before the pool, over the real channels. It covers
every real conv output of a pool window; an absent element -- one in the pool's padding -- is counted nowhere, so count is the number
of present rows x out_c. Each record is fed this model's own previous output."""
import numpy as np

import fcal_ref
import fnet_exact as fe
import fnet_pad as fp


def stats(model, x):
    """The statistic of inputs x [n][in_n] through `model` (cube_import.read_blob form, with or without pads)."""
    recs = fe.conv_records(model)
    s = fcal_ref.empty(len(recs))
    a = np.ascontiguousarray(x, np.float32).reshape(-1, int(np.prod(model["in_shape"])))
    if a.shape[0] == 0:
        return s
    s["absmax"][0], s["hist"][0], s["count"][0] = fcal_ref.of_values(a)
    for i, L in enumerate(recs):
        v, live = fp.pre_activation(L, a)
        s["absmax"][i + 1], s["hist"][i + 1], s["count"][i + 1] = fcal_ref.of_values(v[live])
        a = fp.layer(L, a)
    return s
