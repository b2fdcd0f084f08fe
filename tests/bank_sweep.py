"""The stream-bank sweep: rows chosen so that together they take every path of a push of the stream bank (csrc/edison_stream_bank.hip)
and of the sliding-window core under it (csrc/edison_stream_core.hip) that the number of microphones, the shape of the pushes and the
place in the sliding buffers decide: the shift's rounds with overlapping source and destination, one slot of room, the grid-stride
loops of the MFCC and network launches, the banked filter beyond 256 frames, outputs not asked for, resets at scale.

Test infrastructure, not a test: tests/test_bank_sweep_cpu.py checks that the rows reach every item of full_set() but those in
EXCLUDED, that each row is needed, that the restated buffer sizes are the C++ ones, and walks every row through the emulator below;
tests/test_gpu_bank_sweep.py runs every row on the GPU, exactly.

What a push does on the host side is restated here with the source line of each rule. The launch shapes depend on the CU count
(n_cu): the CPU tests use N_CU, the GPU tests the context's own.

A row is a dict: graph, geom (a name of GEOMS), n_mics, chunk, sched (frames per push), push (dev / host / alt: full pushes from the
host and from the device in turn, ragged ones from the device), alpha, thr (a number or "tie": the reference's own filtered maximum of
one inference), fsm, route (fast / general / spec / lbl), outputs (all / no_softmax / no_logits / none), resets ((push index, microphone
or "all"): done before that push), present (None, or per push None or who the push leaves out: first / last / inner / all / third --
microphone m of push p with (m + p) % 3 == 0 -- or a tuple of microphones; edison_bank_hold.hip and the mask of the filter kernel),
ref (streams: one GeomStream per base recording; independent: no sliding buffer at all)."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256                      # MI355X; the GPU tests pass the context's value
MAX_MICS = 4096                 # ED_STREAM_BANK_MAX_MICS, edison_stream_bank.hip:31
SLOTS, SLOTS_BYTES, SLACK = 8, 64 << 20, 64   # edison_stream_core.h:34-36
EDG_BLOCK, WAVE_TEAM_BYTES = 256, 20480       # mfcc_geom_device.h, edison_kws_geom.hip:19
EDM_G, EDM_WAVES = 4, 8                       # cnn_mfma_kernels.hip:71-72
BASES = 7                       # base recordings of a row with more than 8 microphones: coprime to 4, 8 and 16

# ---- geometries: graph -> the MFCC geometry it is run at. The graph fixes frame_count x num_mfcc only (edison_stream_bank.hip:143).
_SHIPPED = dict(variant="B", frame_len=1024, frame_step=1024, n_samples=32000, mel_nbins=32, first_mfcc=0, num_mfcc=13)
GEOMS = {
    "shipped": ("shipped", _SHIPPED),
    "same_stride": ("same_stride", dict(variant="B", frame_len=800, frame_step=800, n_samples=16000, mel_nbins=40, first_mfcc=1, num_mfcc=12,
                                        lower_edge_hertz=20.0, upper_edge_hertz=4000.0, mel_mtx_scale=64.0)),
    "even_same": ("even_same", dict(variant="B", frame_len=1000, frame_step=500, n_samples=8500, mel_nbins=32, first_mfcc=0, num_mfcc=20, net_input_scale=0.5)),
    "odd_no_softmax": ("odd_no_softmax", dict(variant="B", frame_len=441, frame_step=441, n_samples=11907, mel_nbins=16, first_mfcc=0, num_mfcc=7)),
    # frame_len > 9 x frame_step: at the first shift of a chunk-1 stream (pos = 8) the newest `tail` samples start inside the front
    "square_ov": ("square", dict(variant="A", frame_len=1024, frame_step=100, n_samples=1024 + 63 * 100, mel_nbins=24, first_mfcc=0, num_mfcc=16)),
    # tail = 2304 = 9 x 256: whole rounds; 2560 samples: the workgroup-wide MFCC team
    "shipped_ov256": ("shipped", dict(_SHIPPED, frame_len=2560, frame_step=256, n_samples=2560 + 30 * 256)),
    # an odd frame_len (675 = 27 x 25: the unpacked FFT, workgroup-wide team), 27 frames of 7
    "odd_ov": ("odd_no_softmax", dict(variant="B", frame_len=675, frame_step=64, n_samples=675 + 26 * 64, mel_nbins=16, first_mfcc=0, num_mfcc=7)),
    # frame_len = 31 x frame_step: with the shift at pos = 30 = F - 1 source and destination touch, samples and rows
    "shipped_touch": ("shipped", dict(_SHIPPED, frame_len=3100, frame_step=100, n_samples=3100 + 30 * 100)),
    # one slot: chunk x frame_step > 4 Mi samples. No check bounds frame_step but chunk x frame_step < 2^30 (edison_stream_core.hip:146),
    # so the step is the largest that still leaves a history to shift (below the largest frame_len, 4096) and a multiple of 256
    "shipped_slot1": ("shipped", dict(_SHIPPED, frame_len=4096, frame_step=2048, n_samples=4096 + 30 * 2048)),
    # one frame per window (189 coefficients): no feature history at all
    "odd_f1": ("odd_no_softmax", dict(variant="B", frame_len=1024, frame_step=512, n_samples=1024, mel_nbins=192, first_mfcc=0, num_mfcc=189)),
    # four frames of 256 coefficients: 768 history bytes, whole rounds; tail = 240 < 256
    "square_f4": ("square", dict(variant="A", frame_len=1024, frame_step=784, n_samples=1024 + 3 * 784, mel_nbins=256, first_mfcc=0, num_mfcc=256)),
}

SLOT1_CHUNK = 2049              # the smallest chunk with chunk x 2048 > 4 Mi samples

ROWS = {}


def _row(name, geom, n_mics, chunk=1, sched=None, push="dev", alpha=0.9, thr=0.5, fsm=False, route=None, outputs="all", resets=(),
         ref="streams", present=None):
    graph = GEOMS[geom][0]
    ROWS[name] = dict(graph=graph, geom=geom, n_mics=n_mics, chunk=chunk, sched=list(sched or [1] * 10), push=push, filt=True, alpha=alpha, thr=thr,
                      fsm=fsm, route=route or ("fast" if graph == "shipped" else "general"), outputs=outputs, resets=tuple(resets), ref=ref,
                      present=None if present is None else tuple(present))
    assert present is None or len(present) == len(ROWS[name]["sched"])


# ---- the fast kernel: groups of four microphones per wavefront, eight wavefronts per workgroup
_row("fast_3", "shipped", 3, fsm=True, resets=[(8, 0)])                               # the reset right before the shift (pos = 8)
_row("fast_4", "shipped", 4, push="host", alpha=0.0, resets=[(9, 3)])                 # ... and right after it (pos = 1)
_row("fast_37", "shipped", 37, chunk=3, sched=[3, 3, 1, 3, 3, 2, 3, 3, 3, 3], push="alt", alpha=1.0, fsm=True, outputs="no_softmax",
     resets=[(4, 36)])                                                                # microphone 36: alone in the tenth group
_row("fast_4096", "shipped", 4096, sched=[1] * 9, thr="tie", fsm=True, ref="independent")
# ---- the general matrix-core kernel, forced on the shipped graph: batch x waves = 24 inputs per workgroup
_row("gen_23", "shipped", 23, sched=[1] * 9, route="general", outputs="none")
_row("gen_24", "shipped", 24, chunk=2, sched=[2] * 9, route="general", resets=[(5, "all")])
_row("gen_49", "shipped", 49, sched=[1] * 9, route="general")
_row("spec_49", "shipped", 49, sched=[1] * 9, route="spec")
# one microphone runs ONE launch over a push's windows: a push of more windows than the grid's cap takes (the graph with the smallest
# batch x waves, 22: 5632 at 256 CUs), so a workgroup's loop over inputs comes round; the second push reads behind the first's rows
GEN_CAP_CHUNK = 22 * 256 + 1    # general_cap(N_CU) + 1: the CPU and GPU tests check that it exceeds the cap at their CU count
_row("gen_cap", "square_ov", 1, chunk=GEN_CAP_CHUNK, sched=[GEN_CAP_CHUNK] * 2, ref="independent")
# ---- the layer-by-layer kernel: a workgroup per input, capped at 8 per CU
_row("lbl_4096", "odd_no_softmax", 4096, sched=[1] * 9, route="lbl", outputs="no_logits")
# ---- the shift with overlapping source and destination
_row("square_ov", "square_ov", 1, ref="independent")                                   # one microphone: the single stream's kernels
_row("shipped_ov256", "shipped_ov256", 5, ref="independent")
_row("odd_ov", "odd_ov", 2, ref="independent")
_row("touch", "shipped_touch", 3, chunk=4, sched=[4] * 7 + [2, 4, 4])
# ---- one slot: every push after the first shifts
_row("slot1_single", "shipped_slot1", 1, chunk=SLOT1_CHUNK, sched=[SLOT1_CHUNK] * 3, ref="independent")
_row("slot1_bank", "shipped_slot1", 2, chunk=SLOT1_CHUNK, sched=[SLOT1_CHUNK] * 3, push="host", ref="independent")
# ---- the filter's frame loop beyond 256, 19 classes, a threshold a filtered maximum equals
_row("filt_257", "even_same", 3, chunk=257, sched=[257, 1, 257], alpha=0.6, thr="tie", ref="independent")
# ---- the other class counts and history sizes
_row("same_stride_5", "same_stride", 5, chunk=3, sched=[3, 3, 2, 3, 3, 1, 3, 3, 3, 3], alpha=0.5)
_row("odd_f1", "odd_f1", 3)
_row("square_f4", "square_f4", 3)
# ---- pushes that leave microphones out: the hold kernel's rounds from the top down and the filter kernel's fill
# 16 rows of 20 int8 coefficients: 300 history bytes, a push of n frames holds them up by 20 n -- overlapping below 15 frames, touching
# at 15, disjoint from 16; 19 outputs: from 14 frames on the rows to zero pass 256 bytes and the fill 256 / 19 = 13 rows a round
_row("mask_even", "even_same", 5, chunk=16, sched=[7, 15, 16, 14, 2, 16, 16, 16, 16, 16], push="alt", alpha=0.6, ref="independent",
     resets=[(5, 1)], present=["first", "last", "inner", "all", None, (1, 3), "first", None, "last", "inner"])
_row("mask_257", "even_same", 3, chunk=257, sched=[257, 257], alpha=0.6, ref="independent", present=["inner", "first"])
# 3000 history samples, 100 a frame: held up over themselves by 7 frames, touching by 30 (as the 30 rows of history)
_row("mask_touch", "shipped_touch", 3, chunk=30, sched=[7, 30, 30], fsm=True, ref="independent", present=["first", "last", "inner"])
_row("mask_4096", "shipped", 4096, sched=[1] * 9, fsm=True, ref="independent", present=["third"] * 9)


# ---- the graphs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph_facts(graph):
    """What the launchers need to know of a fixture graph, from the planner itself (edison_net_plan_dump): in_n, n_out, has_softmax,
    the layer-by-layer kernel's LDS bytes and the matrix-core plan's batch, waves and LDS bytes."""
    from edison_amd import _lib, nnom_import
    import plan_emulator as pe
    if graph == "shipped":
        blob = open(_lib.DEFAULT_MODEL, "rb").read()
    else:
        with open(os.path.join(ROOT, "tests", "golden", "alt_models", graph + ".h")) as f:
            blob = nnom_import.build_blob(*nnom_import.parse_weights_h(f.read()))
    p = pe.Plan(blob)
    assert p.M.ok == 1, graph
    return dict(in_n=p.P.in_n, n_out=p.P.out_n, has_softmax=bool(p.P.has_softmax), net_lds=p.P.lds_bytes, batch=p.M.batch, waves=p.M.waves,
                mm_lds=p.M.lds_bytes)


def geometry(name, geoms=None):
    """The KwsGeometry of GEOMS[name] (geoms: another table of the same form)."""
    from edison_amd import _lib
    from edison_amd.kws.geometry import KwsGeometry
    kw = dict((geoms or GEOMS)[name][1])
    kw["variant"] = _lib.MFCC_A if kw["variant"] == "A" else _lib.MFCC_B
    return KwsGeometry.from_config(**kw)


def frame_count(g):
    return g["frame_count"] if g.get("frame_count") else 1 + (g["n_samples"] - g["frame_len"]) // g["frame_step"]


def create_check(row):
    """The create checks that need no device, restated: None, or the reason the bank refuses the row.
    edison_kws_geom.hip:52-69 (ed_kws_geom_check), edison_stream_bank.hip:139-157, edison_stream_core.hip:144-150."""
    g, f = GEOMS[row["geom"]][1], graph_facts(row["graph"])
    if not 1 <= row["n_mics"] <= MAX_MICS:
        return "n_mics must be 1 .. 4096"                                        # edison_stream_bank.hip:139
    if geom_check(g):
        return geom_check(g)
    F = frame_count(g)
    if F * g["num_mfcc"] != f["in_n"]:
        return "frame_count x num_mfcc is not the graph's input"                 # edison_stream_bank.hip:143
    if core_check(row, g):
        return core_check(row, g)
    if row["filt"] and f["n_out"] > 256:
        return "at most 256 outputs"                                             # :151
    if row["fsm"] and f["n_out"] != 10:
        return "the state machine needs 10 outputs"                              # :153
    if row["n_mics"] * row["chunk"] >= 1 << 31:
        return "n_mics x chunk_frames below 2^31"                                # :156
    return None


def geom_check(g):
    """ed_kws_geom_check, edison_kws_geom.hip:52-69."""
    if not 4 <= g["frame_len"] <= 4096:
        return "frame_len 4 .. 4096"                                             # edison_kws_geom.hip:56
    if not 1 <= g["mel_nbins"] <= 256:
        return "mel_nbins 1 .. 256"                                              # :57
    if g["frame_step"] < 1 or g["n_samples"] < g["frame_len"]:
        return "frame_step >= 1, n_samples >= frame_len"                         # :58-59
    F = frame_count(g)
    if (F - 1) * g["frame_step"] + g["frame_len"] > g["n_samples"]:
        return "frames do not fit in n_samples"                                  # :62
    if g["first_mfcc"] < 0 or g["num_mfcc"] < 1 or g["first_mfcc"] + g["num_mfcc"] > g["mel_nbins"]:
        return "first_mfcc + num_mfcc <= mel_nbins"                              # :64
    return None


def core_check(row, g):
    """ed_stream_core_check_opts, edison_stream_core.hip:144-150."""
    if row["chunk"] < 1:
        return "chunk_frames >= 1"                                               # edison_stream_core.hip:144
    if row["chunk"] * g["frame_step"] >= 1 << 30:
        return "chunk_frames x frame_step below 2^30"                            # :146
    if row["fsm"] and not row["filt"]:
        return "fsm needs the filter"                                            # :148
    if row["filt"] and not 0.0 <= row["alpha"] <= 1.0:
        return "alpha within [0, 1]"                                             # :149
    return None


# ---- the core's sizes ------------------------------------------------------------------------------------------------------------
def sizes(row, feat_elem=1, geoms=None):
    """slots from the 64 MB rule, then one microphone's buffers: edison_stream_core.hip:159, 172-176, edison_stream_core.h:41-45.
    feat_elem: bytes per feature element, 1 for the int8 graph, 4 for the float network (geoms: its table of geometries)."""
    g = (geoms or GEOMS)[row["geom"]][1]
    hop, chunk, nm = g["frame_step"], row["chunk"], g["num_mfcc"]
    F = frame_count(g)
    tail = g["frame_len"] - hop if g["frame_len"] > hop else 0                   # edison_stream_core.hip:159
    slots = SLOTS if chunk * hop * 2 * SLOTS <= SLOTS_BYTES else 1               # :173
    return dict(F=F, nm=nm, hop=hop, N=g["frame_len"], tail=tail, chunk=chunk, slots=slots, n_mics=row["n_mics"],
                mic_audio=tail + slots * chunk * hop,                            # edison_stream_core.h:41
                mic_feat=feat_elem * (F - 1 + slots * chunk) * nm,               # :42-45, in bytes
                feat_bytes=feat_elem * (F - 1) * nm)                             # edison_stream_core.hip:135


def window_addr(s, pos, i, m):
    """Byte offset in d_feat of window i of a push for microphone m: edison_stream_bank.hip:70, 89 (win + i * nm, stride mic_feat; one microphone: :81, win at a stride of nm)."""
    return m * s["mic_feat"] + (pos + i) * s["nm"]


def out_index(i, m, n_mics):
    """Row of the time-major outputs: slab i of the push, microphone m (edison_stream_bank.hip:86-90; the filter: edison_stream_core.hip:80 `i * n_mics + m`)."""
    return i * n_mics + m


def base_of(m, n_mics):
    """The base recording microphone m plays: its own up to 8 microphones, else one of BASES such that neighbours differ."""
    return m if n_mics <= 8 else (3 * m + m // BASES) % BASES


# ---- the launches of a push --------------------------------------------------------------------------------------------------------
def mfcc_team(g):
    """edison_kws_geom.hip:156-166: the LDS slice of a frame decides between a wavefront and the workgroup."""
    N, nmel = g["frame_len"], g["mel_nbins"]
    M = N // 2 if N % 2 == 0 else N
    m = M
    for r in (4, 2, 3, 5):
        while m % r == 0:
            m //= r
    nb = N // 2 if g["variant"] == "A" else N // 2 + 1
    r0, r1 = (2 * M, 2 * M) if m == 1 else ((N + 1) & ~1, (nb + 1) & ~1)
    words = r0 + r1 + ((nmel + 1) & ~1)
    return (64 if 8 * words <= WAVE_TEAM_BYTES else EDG_BLOCK), words


def mfcc_launch(g, n_frames, n_cu):
    """edg_launch_shape, mfcc_geom_device.h:98-112, and the frame loop mfcc_geom_frames.inc:19."""
    team, words = mfcc_team(g)
    teams = EDG_BLOCK // team
    per_cu = max(1, min(4, (160 * 1024) // (8 * teams * words)))
    blocks = min(-(-n_frames // teams), per_cu * n_cu)
    return dict(team=team, blocks=blocks, wraps=n_frames > blocks * teams)


def net_launch(row, n_cu, frames=1):
    """A network launch of a push of `frames` frames (edison_stream_bank.hip:79-93): one per frame over its n = n_mics windows, or, with
    one microphone, ONE over the push's n = frames windows. Grid and whether the kernel's loop over inputs wraps."""
    f, n = graph_facts(row["graph"]), row["n_mics"] if row["n_mics"] > 1 else frames
    if row["route"] == "fast":          # ed_launch_cnn_mfma_flag, cnn_mfma_kernels.hip:810-812; a wave draws groups from its workgroup's slice (:267)
        groups = -(-n // EDM_G)
        blocks = min(-(-groups // EDM_WAVES), n_cu)
        return dict(kernel="fast", blocks=blocks, wraps=groups > blocks * EDM_WAVES, unit=EDM_G)
    if row["route"] in ("general", "spec"):   # ed_launch_net_mfma, cnn_net_mfma_kernels.hip:1366-1371 (edison_net_jit.hip:483: the same grid)
        per_cu = max(1, min((160 * 1024) // (f["mm_lds"] + 256), 32 // f["waves"]))
        per_block = f["batch"] * f["waves"]
        blocks = min(-(-n // per_block), n_cu * per_cu)
        return dict(kernel=row["route"], blocks=blocks, wraps=n > blocks * per_block, unit=per_block, cap=n_cu * per_cu * per_block)
    per_cu = max(1, min(8, (160 * 1024) // (f["net_lds"] + 256))) if f["net_lds"] > 0 else 8    # ed_launch_net, cnn_net_kernels.hip:400-404
    blocks = min(n, n_cu * per_cu)
    return dict(kernel="lbl", blocks=blocks, wraps=n > blocks, unit=1)                            # :344 u += gridDim.x


def _band(v):
    return "0" if v == 0 else ("<256" if v < 256 else ("x256" if v % 256 == 0 else ">256"))


# ---- the emulator ------------------------------------------------------------------------------------------------------------------
POISON, GARBAGE = -1, -2        # never written; the samples and rows of a microphone the push left out


def shift_rounds(buf, src, count):
    """The kernels' rounds of 256 (edison_stream_core.hip:22-37, a workgroup per microphone): all read, barrier, all write."""
    for base in range(0, count, 256):
        hi = min(base + 256, count)
        v = buf[src + base:src + hi].copy()
        buf[base:hi] = v


def shift_unordered(buf, src, count):
    """The same elements moved by wavefronts that nothing orders -- no barrier, so a later wavefront may run rounds ahead of an earlier
    one. The schedule that shows it: pieces of 64 from the last to the first, each read and then written."""
    for base in range((count - 1) // 64 * 64, -1, -64):
        hi = min(base + 64, count)
        buf[base:hi] = buf[src + base:src + hi].copy()


def shift_forward64(buf, src, count):
    """One wavefront, no barrier: pieces of 64 in ascending order. The destination lies below the source, so an ascending copy only
    overwrites what it has read: this one is CORRECT whatever the overlap (the CPU test shows it on every row)."""
    for base in range(0, count, 64):
        hi = min(base + 64, count)
        buf[base:hi] = buf[src + base:src + hi].copy()


def hold_rounds(buf, src, count, by):
    """hold_up, edison_bank_hold.hip:20-30: `count` elements from src up by `by`, rounds of 256 from the top down, all read, barrier, all write."""
    for top in range(count, 0, -256):
        lo = max(0, top - 256)
        v = buf[src + lo:src + top].copy()
        buf[src + by + lo:src + by + top] = v


def hold_ascending(buf, src, count, by):
    """The same rounds from the bottom up, as the shift kernel runs its own: WRONG when the destination overlaps the source, for a
    round's writes land on elements a later round has yet to read."""
    for base in range(0, count, 256):
        hi = min(base + 256, count)
        v = buf[src + base:src + hi].copy()
        buf[src + by + base:src + by + hi] = v


def absent_of(row, p):
    """The microphones push p of the row leaves out (sorted list; empty: the push carries no mask or an all-ones one)."""
    pat, M = (row.get("present") or [None] * len(row["sched"]))[p], row["n_mics"]
    if pat is None:
        return []
    if isinstance(pat, tuple):
        return sorted(pat)
    return {"first": [0], "last": [M - 1], "inner": [M // 2], "all": list(range(M)), "third": [m for m in range(M) if (m + p) % 3 == 0]}[pat]


def fill_rows(n, n_out):
    """The rows of filt the absent fill writes for one microphone, by the kernel's loop (edison_stream_core.hip:62-63): lane t serves
    element t % n_out of rows t / n_out, + per, ... while t / n_out < per = 256 / n_out. Returns the [n][n_out] mask of written elements."""
    done = np.zeros((n, n_out), bool)
    per = 256 // n_out
    for t in range(256):
        r, c = divmod(t, n_out)
        if r < per:
            done[r:n:per, c] = True
    return done


def hold_and_fill(s, n_out, row_bytes, feat_elem, a_of, f_of, pos, n, absent, items, problems, p, hold, variant, shifted, reset_now):
    """What a masked push does behind its launches, for both banks (ed_stream_core_finish_push_present, edison_stream_core.hip:338-361):
    the hold of every absent microphone's history up by the push's advance, then the filter kernel's fill. Adds the items reached and
    the problems: a row of the fill not written, or written for a present microphone. a_of(m) / f_of(m): microphone m's samples and
    feature bytes (None: a microphone the walk does not keep)."""
    M, A, FB, tail, hop, nm = s["n_mics"], s["mic_audio"], s["mic_feat"], s["tail"], s["hop"], s["nm"]
    a_src, a_by, f_src, f_by = pos * hop, n * hop, pos * nm * feat_elem, n * nm * feat_elem         # :351-353
    for what, count, by in (("samples", tail, a_by), ("rows", s["feat_bytes"], f_by)):
        if count and absent:
            items.add(("hold", what, "overlapping" if by < count else "touching" if by == count else "disjoint"))
    for m in absent:
        assert a_src + a_by + tail <= A and f_src + f_by + s["feat_bytes"] <= FB, "the hold leaves the microphone's buffers"
        if a_of(m) is not None:
            hold(a_of(m), a_src, tail, a_by)
            hold(f_of(m), f_src, s["feat_bytes"], f_by)
    if absent:
        items.add(("hold zero", "<=256 bytes" if n * row_bytes <= 256 else ">256 bytes"))          # edison_bank_hold.hip:42
        items.add(("fill", "n > 256" if n > 256 else "one round" if n <= 256 // n_out else "several rounds"))
        if M == MAX_MICS:
            items.add(("hold grid", "4096"))                                                         # edison_bank_hold.hip:55
        for m in absent:
            items.add(("absent", "first" if m == 0 else "last" if m == M - 1 else "inner"))
        if len(absent) == M:
            items.add(("absent", "everyone"))
        if shifted:
            items.add(("absent", "through a shift"))
        if reset_now & set(absent):
            items.add(("absent", "reset while absent"))
        full = fill_rows(n, n_out)
        assert all(i in range(n) for i in range(0, n, 256))                                          # :65-71 i = t, t + 256, ...
        filled = set(absent) if variant != "fill_present" else set(range(M)) - set(absent)
        for m in (range(M) if M <= 64 else sorted(set(absent[:2] + absent[-2:] + [0, 1, M - 2, M - 1]))):
            if (m in filled) != (m in absent) or (m in absent and not full.all()):
                problems.append(("fill", p, m))


MASKED_ROW_ITEMS = ("hold", "hold zero", "hold grid", "fill", "absent", "masked filter", "shift", "overlap", "reset", "reset_mic", "residue")


def _tok(m, epoch, kind, j):
    """An opaque value for element j of microphone m's zero-led stream since its reset number `epoch`: kind 0 a sample, 1 a feature."""
    return (((m * 64 + epoch) * 2 + kind) << 32) + j


def walk(row, n_cu=N_CU, shift=shift_rounds, variant=None, check=True, hold=hold_rounds):
    """Walks the row's push schedule through the core with numpy buffers of tokens. Returns (items, problems): the coverage items the
    walk reached, and what a consumer would have read wrong (empty for the real rules). `variant` swaps one rule for a mis-reading:
    mic_major, shared_state, one_machine, window_stride, fill_present (the fill written to the present microphones). A microphone's tokens
    count the frames of its own stream -- those of the pushes it was present in -- so a push it was absent from must leave no trace. Reads
    outside a microphone's buffers plus the slack raise."""
    s = sizes(row)
    g = GEOMS[row["geom"]][1]
    F, nm, hop, N, tail, M = s["F"], s["nm"], s["hop"], s["N"], s["tail"], s["n_mics"]
    A, FB = s["mic_audio"], s["mic_feat"]
    audio = np.full(M * A + SLACK // 2, POISON, np.int64)
    feat = np.full(M * FB + SLACK, POISON, np.int64)
    epoch, cnt = [0] * M, [0] * M                # per microphone: resets so far, frames of its own stream since the last one
    seen, pos = 0, 0
    items, problems = set(), []
    owner = np.arange(M)                         # whose filter state / machine entry m of d_state / d_fsm is
    shifted = False                              # the push before this one moved the history
    fast = row["route"] == "fast"

    def start_state(m):                          # start_state, edison_stream_core.hip:220-245, at the current pos
        epoch[m] += 1
        cnt[m] = 0
        audio[m * A + pos * hop:m * A + pos * hop + tail] = _tok(m, epoch[m], 0, 0) + np.arange(tail)
        feat[m * FB + pos * nm:m * FB + pos * nm + (F - 1) * nm] = _tok(m, epoch[m], 1, 0) + np.arange((F - 1) * nm)

    for m in range(M):
        start_state(m)
    resets = dict()
    for at, who in row["resets"]:
        resets.setdefault(at, []).append(who)
    items |= {("slots", s["slots"], "single" if M == 1 else "bank"), ("tail", _band(tail)), ("feat_bytes", _band(s["feat_bytes"])),
              ("frame_len", "odd" if N % 2 else "even"), ("n_out", graph_facts(row["graph"])["n_out"]), ("alpha", {0.0: "0", 1.0: "1"}.get(row["alpha"], "interior")),
              ("threshold", "tie" if row["thr"] == "tie" else "plain"), ("fsm", row["fsm"]), ("outputs", row["outputs"]), ("push", row["push"]),
              ("ref", row["ref"], "large" if M > 8 else "small")}
    # the inputs of one network launch: the microphones, or one microphone's frames of the push
    for k in ({M} if M > 1 else set(row["sched"])):
        nl = net_launch(row, n_cu, k)
        if nl["kernel"] == "fast":
            items.add(("fast", "<4" if k < 4 else "4" if k == 4 else "4096" if k == MAX_MICS else "ragged" if k % 4 else "whole"))
            if -(-k // EDM_G) > EDM_WAVES:
                items.add(("fast", "more than one workgroup"))
        elif nl["kernel"] == "general":
            if nl["wraps"]:     # the grid at its cap, a workgroup's loop comes round: not the one-pass grids the other items tell apart
                items.add(("general", "blocks above the cap"))
            else:
                items.add(("general", "under" if k < nl["unit"] else "equal" if k == nl["unit"] else "over ragged" if k % nl["unit"] else "over whole"))
        elif nl["kernel"] == "spec":
            if nl["blocks"] > 1:
                items.add(("spec", "more than one workgroup"))
        elif nl["wraps"]:
            items.add(("lbl", "block loop wraps"))

    for p, n in enumerate(row["sched"]):
        absent, reset_now = absent_of(row, p), set()
        gone = set(absent)
        for who in resets.get(p, ()):
            will_shift = not (pos + n <= s["slots"] * s["chunk"] or pos == 0)
            if who == "all":                     # ed_stream_core_reset, :258-274: pos = 0, every microphone, frames_seen = 0
                pos = seen = 0
                for m in range(M):
                    start_state(m)
                items.add(("reset", "all"))
            else:
                start_state(who)
                reset_now.add(who)
                assert pos != 0
                items.add(("reset_mic", "first" if who == 0 else "last" if who == M - 1 else "inner"))
                if M % 4 and who >= M - M % 4:
                    items.add(("reset_mic", "in a ragged last group"))
                items.add(("reset_mic", "right before a shift" if will_shift else "right after a shift" if shifted else "elsewhere"))
        assert 1 <= n <= s["chunk"]              # begin_push, :278
        # make_room, edison_stream_core.hip:131-140
        if not (pos + n <= s["slots"] * s["chunk"] or pos == 0):
            a_src, f_src = pos * hop, pos * nm
            for what, src, count in (("samples", a_src, tail), ("rows", f_src, s["feat_bytes"])):
                if count:
                    items.add(("shift", what, "single" if M == 1 else "bank", "overlapping" if src < count else "touching" if src == count else "disjoint"))
                    if src < count and M > 1:
                        items.add(("overlap", what, _band(count)))
            for m in range(M):
                shift(audio[m * A:(m + 1) * A], a_src, tail)
                shift(feat[m * FB:(m + 1) * FB], f_src, s["feat_bytes"])
            pos = 0
            shifted = True
        else:
            shifted = False
        # the upload: d_audio + pos * hop + tail of every microphone, :281-287
        for m in range(M):
            at = m * A + pos * hop + tail
            assert at + n * hop <= (m + 1) * A
            audio[at:at + n * hop] = GARBAGE if m in gone else _tok(m, epoch[m], 0, tail + cnt[m] * hop) + np.arange(n * hop)
        # ONE MFCC launch over n_mics * n frames: edison_stream_bank.hip:71-78, mfcc_geom_frames.inc:19-22, mfcc_geom_kernels.hip:29-33
        ml = mfcc_launch(g, M * n, n_cu)
        items |= {("mfcc", "team", ml["team"]), ("mfcc", "wraps" if ml["wraps"] else "one pass"), ("mfcc", "frames_per_utt", "1" if n == 1 else "chunk" if n == s["chunk"] else "ragged")}
        feat_skip = FB - n * nm
        for gi in range(M * n):
            u, f = divmod(gi, n)
            x0 = pos * hop + u * A + f * hop
            assert u * A <= x0 and x0 + N <= (u + 1) * A, "frame outside its microphone's samples"
            if check and u not in gone and (gi < 2 * n or gi >= (M - 2) * n):          # every frame of the first and last microphones
                want = _tok(u, epoch[u], 0, (cnt[u] + f) * hop) + np.arange(N)
                if not np.array_equal(audio[x0:x0 + N], want):
                    problems.append(("samples", p, u, f))
            o = pos * nm + (F - 1) * nm + gi * nm + feat_skip * u
            assert u * FB <= o and o + nm <= (u + 1) * FB, "row outside its microphone's rows"
            feat[o:o + nm] = GARBAGE if u in gone else _tok(u, epoch[u], 1, (F - 1 + cnt[u] + f) * nm) + np.arange(nm)
        # n network launches over the n_mics windows of a frame, or one microphone's ONE over its n windows: edison_stream_bank.hip:79-93
        stride = FB + (nm if variant == "window_stride" else 0)
        full = pos + n == s["slots"] * s["chunk"]
        for i in range(n):
            for m in range(M):
                at = m * stride + (pos + i) * nm
                if variant is None:
                    assert at == window_addr(s, pos, i, m)
                lo, hi = at, at + F * nm
                if fast:                          # edm_load_rows, cnn_mfma_kernels.hip:170-186: 16 bytes per 13-byte row, the batch's last row 3 early
                    items.add(("residue", at % 16))
                    hi = hi if (m == M - 1 if M > 1 else i == n - 1) else hi + 3
                    if variant is None and full and i == n - 1 and m == M - 1:
                        assert hi == M * FB
                        items.add(("fast", "last window ends the buffers"))
                if variant is not None and hi > M * FB + SLACK:
                    problems.append(("window", p, m, i))
                    continue
                assert 0 <= lo and hi <= M * FB + SLACK, "window outside the rows and their slack"
                if check and m not in gone and (m < 2 or m >= M - 2 or m % 97 == 0):
                    want = _tok(m, epoch[m], 1, (cnt[m] + i) * nm) + np.arange(F * nm)
                    if not np.array_equal(feat[at:at + F * nm], want):
                        problems.append(("window", p, m, i))
        # the filter (+ machine), a workgroup per microphone: edison_stream_core.hip:52-111, over slab-major entries
        masked = bool(row.get("present")) and row["present"][p] is not None      # the kernel's mask branch, edison_stream_core.hip:58
        items.add(("masked filter" if masked else "filter", "n", "1" if n == 1 else ">256" if n > 256 else "ragged" if n < s["chunk"] else "chunk"))
        if n > 1 and M > 1:
            assert n != M
            entry = np.full(n * M, POISON, np.int64)
            for i in range(n):
                for m in range(M):
                    entry[out_index(i, m, M)] = m * (1 << 32) + seen + i
            for m in range(M):
                # state[m * n_out + t] and fs.fsm[m], :77, :102
                if owner[0 if variant == "shared_state" else m] != m or owner[0 if variant == "one_machine" else m] != m:
                    problems.append(("state", p, m))
                for i in range(n):
                    if entry[m * n + i if variant == "mic_major" else out_index(i, m, M)] != m * (1 << 32) + seen + i:
                        problems.append(("filter", p, m, i))
                        break
        if row.get("present") and row["present"][p] is not None:
            f = graph_facts(row["graph"])
            hold_and_fill(s, f["n_out"], f["n_out"], 1, lambda m: audio[m * A:(m + 1) * A], lambda m: feat[m * FB:(m + 1) * FB], pos, n, absent, items,
                          problems, p, hold, variant, shifted, reset_now)
        pos += n
        seen += n
        for m in range(M):
            cnt[m] += 0 if m in gone else n
    if row.get("present"):
        # a row with masks is in the sweep for its holds and fills: what else it reaches, the rows without a mask are there for
        items = {it for it in items if it[0] in MASKED_ROW_ITEMS}
    return items, problems


def is_overlap_row(row):
    """Some shift of the row's schedule moves samples or rows onto their own source."""
    return any(it[0] == "shift" and it[3] == "overlapping" for it in walk(row, check=False)[0])


def is_hold_overlap_row(row):
    """Some masked push of the row holds samples or rows up onto their own source."""
    return any(it[0] == "hold" and it[2] == "overlapping" for it in walk(row, check=False)[0])


def mask_set():
    """The items of pushes that leave microphones out."""
    s = {("hold", w, k) for w in ("samples", "rows") for k in ("overlapping", "touching", "disjoint")}
    s |= {("hold zero", "<=256 bytes"), ("hold zero", ">256 bytes"), ("hold grid", "4096")} | {("fill", v) for v in ("one round", "several rounds", "n > 256")}
    s |= {("masked filter", "n", v) for v in ("1", "ragged", ">256", "chunk")}
    return s | {("absent", v) for v in ("first", "last", "inner", "everyone", "through a shift", "reset while absent")}


def full_set():
    """Every item a row could reach."""
    s = {("slots", n, k) for n in (1, 8) for k in ("single", "bank")}
    s |= {(k, b) for k in ("tail", "feat_bytes") for b in ("0", "<256", ">256", "x256")}
    s |= {("frame_len", "odd"), ("frame_len", "even")} | {("n_out", n) for n in (5, 7, 10, 19)} | {("alpha", a) for a in ("0", "1", "interior")}
    s |= {("threshold", "tie"), ("threshold", "plain"), ("fsm", True), ("fsm", False)} | {("outputs", o) for o in ("all", "no_softmax", "no_logits", "none")}
    s |= {("push", p) for p in ("dev", "host", "alt")} | {("ref", "independent", "large"), ("ref", "independent", "small"), ("ref", "streams", "large"), ("ref", "streams", "small")}
    s |= {("fast", v) for v in ("<4", "4", "ragged", "4096", "more than one workgroup", "last window ends the buffers")}
    s |= {("general", v) for v in ("under", "equal", "over ragged", "blocks above the cap")} | {("spec", "more than one workgroup"), ("lbl", "block loop wraps")}
    s |= {("reset", "all")} | {("reset_mic", v) for v in ("first", "last", "inner", "in a ragged last group", "right before a shift", "right after a shift", "elsewhere")}
    s |= {("shift", w, "bank", k) for w in ("samples", "rows") for k in ("overlapping", "touching", "disjoint")}
    s |= {("shift", w, "single", k) for w in ("samples", "rows") for k in ("overlapping", "disjoint")}
    s |= {("overlap", "samples", ">256"), ("overlap", "samples", "x256"), ("overlap", "rows", "<256"), ("overlap", "rows", ">256")}
    s |= {("mfcc", "team", 64), ("mfcc", "team", EDG_BLOCK), ("mfcc", "wraps"), ("mfcc", "one pass")} | {("mfcc", "frames_per_utt", v) for v in ("1", "ragged", "chunk")}
    s |= {("residue", r) for r in range(16)} | {("filter", "n", v) for v in ("1", "ragged", ">256", "chunk")}
    s |= {("n_mics", ">4096"), ("n_mics x chunk", ">=2^31")}
    return s | mask_set()


# item -> the host check or launch rule that keeps every accepted bank from it
EXCLUDED = {
    ("n_mics", ">4096"): "edison_stream_bank.hip:139 refuses n_mics outside 1 .. 4096 (tests/test_gpu_stream_bank.py::test_errors runs it)",
    ("n_mics x chunk", ">=2^31"): "edison_stream_bank.hip:156 refuses it, and no allocation reaches it: 2^31 frames of at least one sample each are 4 GB of "
                                  "samples per push, which edison_stream_core.hip:146 (chunk x frame_step < 2^30) and HBM rule out for 4096 microphones",
}


def general_cap(n_cu):
    """The fewest inputs at which a fixture graph's general-kernel grid reaches its cap (cnn_net_mfma_kernels.hip:1371: n_cu x per_cu
    workgroups of batch x waves inputs): 5632 at 256 CUs, which a launch per frame stays under (edison_stream_bank.hip:139 admits 4096
    microphones) and one microphone's launch over a push's windows passes where the push has more (row gen_cap)."""
    return min(net_launch(dict(graph=gname, n_mics=1, route="general"), n_cu)["cap"] for gname in ("shipped", "square", "odd_no_softmax", "same_stride", "even_same"))
