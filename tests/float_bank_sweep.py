"""The float-bank sweep: rows chosen so that together they take every path of a push of the float bank (csrc/edison_float_bank.hip), of
the sliding-window core under it with float32 rows (csrc/edison_stream_core.hip, feat_elem = 4) and of a push that leaves microphones
out (csrc/edison_bank_hold.hip, the mask branch of the filter kernel) that the number of microphones, the shape of the pushes, the class
count and the place in the sliding buffers decide.

Test infrastructure, not a test, in the style of tests/bank_sweep.py, from which it takes what is restated there already (the core's
sizes, the shift's rounds, the hold's rounds, the fill, the MFCC launch shape): tests/test_float_bank_sweep_cpu.py checks that the rows
reach every item of full_set() but those in EXCLUDED, that each row is needed, that the restated sizes are the C++ ones, and walks every
row through the emulator below; tests/test_gpu_float_bank_sweep.py runs every row on the GPU, exactly.

A row is a dict: net ("fixture": tests/golden/cube_kws.ednf, or the class count of a network generated with cube_synth.cube_sources at
the row's geometry), geom (a name of GEOMS), q15 (the firmware flow), n_mics, chunk, sched (frames per push), push (dev / host / alt, as
bank_sweep), alpha, thr (a number or "tie"), fsm, outputs (all / no_probs / no_logits / none: what a device push is given pointers
for), clip (lo, hi), resets, present (as bank_sweep), ref (independent: no stream, no bank and none of the core's kernels; streams: one
FloatStream per base recording and per reset)."""
import functools
import os

import numpy as np

import bank_sweep as bs
from bank_sweep import (BASES, GARBAGE, MAX_MICS, N_CU, POISON, SLACK, _band, _tok, absent_of, base_of, frame_count, hold_and_fill, hold_ascending,  # noqa: F401
                        hold_rounds, mfcc_launch, shift_forward64, shift_rounds, shift_unordered)

ROOT = bs.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "cube_kws.ednf")
FEAT_ELEM = 4                   # sizeof(float): ed_stream_core_create(.., sizeof(float), sizeof(float), ..), edison_float_bank.hip:182
EQ_WPB = 16                     # frames in flight per workgroup of the variant C kernel, mfcc_q15_kernels.hip:52
DEFAULT_CLIP = (-32768.0, 32767.0)

_G = {k: v[1] for k, v in bs.GEOMS.items()}
GEOMS = {k: (k, _G[k]) for k in ("shipped", "even_same", "square_ov", "shipped_touch", "shipped_slot1", "odd_f1")}
# 16 rows of history of 16 floats: 1024 bytes, whole rounds; frame_len > 9 x frame_step, so samples and rows overlap at pos = 8
GEOMS["ov_x256"] = ("ov_x256", dict(variant="B", frame_len=1024, frame_step=64, n_samples=1024 + 16 * 64, mel_nbins=16, first_mfcc=0, num_mfcc=16))
# 112 history samples and 96 history bytes: one ragged round each
GEOMS["tiny"] = ("tiny", dict(variant="B", frame_len=512, frame_step=400, n_samples=512 + 3 * 400, mel_nbins=8, first_mfcc=0, num_mfcc=8))
# the firmware flow's framing with a short window: 4 frames of 13
GEOMS["q15_f4"] = ("q15_f4", dict(bs._SHIPPED, n_samples=4 * 1024))

ROWS = {}


def _row(name, geom, net, n_mics, q15=False, chunk=1, sched=None, push="dev", alpha=0.5, thr=0.5, fsm=False, outputs="all", clip=DEFAULT_CLIP,
         resets=(), present=None, ref="independent"):
    ROWS[name] = dict(net=net, geom=geom, q15=q15, n_mics=n_mics, chunk=chunk, sched=list(sched or [1] * 10), push=push, filt=True, alpha=alpha,
                      thr=thr, fsm=fsm, outputs=outputs, clip=clip, resets=tuple(resets), present=None if present is None else tuple(present), ref=ref)
    assert present is None or len(present) == len(ROWS[name]["sched"])


# ---- tiles of the network launch (16 utterances with the generated networks, 7 with the fixture), both flows
_row("host_3x3", "even_same", 6, 3, chunk=3, sched=[3, 3, 2, 3, 3, 3, 3, 3, 3, 3], push="alt", clip=(-2.0, 2.0))   # 9 and 6 windows: under
_row("q15_4x4", "shipped", 10, 4, q15=True, chunk=4, sched=[4] * 9, push="host", fsm=True, resets=[(2, 1), (5, "all")], ref="streams")   # 16: equal
_row("host_17x2", "square_ov", 6, 17, chunk=2, sched=[2] * 9, outputs="none")       # 34: ragged, tile 1 straddles; rows overlap at pos = 16
_row("host_4096x3", "tiny", 10, 4096, chunk=3, sched=[3, 3], outputs="no_logits", fsm=True)   # 768 whole tiles, the MFCC grid wraps
_row("q15_4096x3", "q15_f4", 10, 4096, q15=True, chunk=3, sched=[3])               # 12288 frames: the variant C grid at its cap
_row("q15_single", "q15_f4", 6, 1, q15=True, chunk=3, sched=[3, 2, 3])                # one microphone: variant C writes in place
# ---- the shift with float rows
_row("ov_single", "square_ov", 10, 1)                                               # one microphone: in place, by frame
_row("ov_x256_5", "ov_x256", 6, 5, outputs="no_probs")
_row("touch", "shipped_touch", 10, 3, chunk=4, sched=[4] * 7 + [2, 4, 4])
_row("f1", "odd_f1", 6, 3, alpha=1.0)                                               # no row history
_row("tiny", "tiny", 1, 3, alpha=0.0)                                               # one class; ragged rounds below 256
# ---- one slot
_row("slot1_single", "shipped_slot1", 10, 1, chunk=bs.SLOT1_CHUNK, sched=[bs.SLOT1_CHUNK] * 3)
_row("slot1_bank", "shipped_slot1", 10, 2, chunk=bs.SLOT1_CHUNK, sched=[bs.SLOT1_CHUNK] * 3, push="host")
# ---- the fixture network, resets against streams
_row("reset_before", "shipped", "fixture", 3, fsm=True, resets=[(8, 0)], ref="streams")
_row("reset_after", "shipped", "fixture", 8, q15=True, push="host", fsm=True, resets=[(9, 7)], ref="streams")   # 8 > 7: a ragged second tile
# ---- the filter beyond 256 frames at 256 classes, a tie, and masks whose fill runs 257 rounds
_row("filt_257", "even_same", 256, 3, chunk=257, sched=[257, 1, 257], alpha=0.6, thr="tie", present=[None, "inner", "first"])
# ---- pushes that leave microphones out: 15 rows of history of 20 floats, a push of n frames holds them up by 80 n bytes
_row("mask_even", "even_same", 10, 5, chunk=26, sched=[7, 15, 16, 26, 2, 26, 26, 26, 26, 26, 26], push="alt", fsm=True, resets=[(5, 1)],
     present=["first", "last", "inner", "all", None, (1, 3), "first", None, "last", "first", "inner"])
_row("mask_200", "even_same", 200, 4, chunk=2, sched=[2] * 4, present=["first", None, "last", "inner"])
_row("mask_touch", "shipped_touch", 10, 3, chunk=30, sched=[7, 30, 30], fsm=True, present=["first", "last", "inner"])
_row("mask_4096", "shipped", 10, 4096, q15=True, sched=[1] * 9, fsm=True, present=["third"] * 9)


# ---- the networks ----------------------------------------------------------------------------------------------------------------
def _specs(F, nm, n_out):
    conv = [("conv", 4, (3, 3), (1, 1), (2, 2), 1)] if F >= 4 and nm >= 4 else []
    return conv + [("dense", 16), ("relu",), ("dense", n_out), ("softmax",)]


@functools.lru_cache(maxsize=None)
def blob_of(net, geom):
    """The .ednf bytes of a row's network."""
    if net == "fixture":
        with open(FIXTURE, "rb") as f:
            return f.read()
    import tempfile
    import cube_synth
    from edison_amd import cube_import
    g = GEOMS[geom][1]
    sources = cube_synth.cube_sources((frame_count(g), g["num_mfcc"], 1), _specs(frame_count(g), g["num_mfcc"], net), seed=net)
    with tempfile.TemporaryDirectory() as d:
        for fname, text in zip(("n.c", "n_data.c"), sources):
            with open(os.path.join(d, fname), "w") as f:
                f.write(text)
        return cube_import.import_files(os.path.join(d, "n.c"), os.path.join(d, "n_data.c"))


@functools.lru_cache(maxsize=None)
def plan_of(net, geom):
    """fnet_plan.plan of the row's network: in_n, n_out, batch (the utterances of a tile)."""
    import fnet_plan
    p = fnet_plan.plan(blob_of(net, geom))
    assert "error" not in p, (net, geom, p)
    return p


def geometry(row):
    return bs.geometry(row["geom"], GEOMS)


def sizes(row):
    return bs.sizes(row, FEAT_ELEM, GEOMS)


def create_check(row):
    """The create checks that need no device, restated: None, or the reason the bank refuses the row. edison_float_bank.hip:152-171,
    edison_fnet.hip:304-332 (kws_float_check), edison_kws_geom.hip:52-69, edison_stream_core.hip:144-150."""
    g, pl = GEOMS[row["geom"]][1], plan_of(row["net"], row["geom"])
    if not 1 <= row["n_mics"] <= MAX_MICS:
        return "n_mics must be 1 .. 4096"                                        # edison_float_bank.hip:152
    if not row["clip"][0] <= row["clip"][1]:
        return "clip_lo > clip_hi"                                               # edison_fnet.hip:306
    if row["q15"] and not (g["frame_len"] == g["frame_step"] == 1024 and g["mel_nbins"] == 32 and g["first_mfcc"] == 0 and 1 <= g["num_mfcc"] <= 32):
        return "q15 = 1 takes the shipped geometry only"                         # :310-312
    if bs.geom_check(g):
        return bs.geom_check(g)                                                  # :321 (q15: :313-316, the same bounds)
    if frame_count(g) * g["num_mfcc"] != pl["in_n"]:
        return "frame_count x num_mfcc is not the network's input"               # :326
    if bs.core_check(row, g):
        return bs.core_check(row, g)                                             # edison_float_bank.hip:165
    if row["filt"] and pl["n_out"] > 256:
        return "at most 256 outputs"                                             # :149
    if row["fsm"] and pl["n_out"] != 10:
        return "the state machine needs 10 outputs"                              # :150
    if row["n_mics"] * row["chunk"] >= 1 << 31:
        return "n_mics x chunk_frames below 2^31"                                # :153
    return None


def q15_grid(n_frames, n_cu):
    """ed_launch_q15_shape, mfcc_q15_kernels.hip:693-695: a workgroup per EQ_WPB frames, capped at n_cu x blocks_per_cu. The occupancy
    query answers 1: a workgroup's LDS (EQ_LDS_DWORDS, :414: over 16 x 1872 dwords) is more than half of a CU's 160 KB."""
    blocks = -(-n_frames // EQ_WPB)
    return dict(blocks=min(blocks, n_cu), capped=blocks > n_cu)


def net_launch(row, n):
    """edison_float_bank.hip:98-100: which launch serves a push of n frames, and its utterances in output order as (frame, microphone)."""
    M = row["n_mics"]
    if M == 1:
        return "by_frame", n                                                     # ed_launch_fnet over n windows num_mfcc floats apart
    if n == 1:
        return "by_microphone", M                                                # ... over n_mics windows mic_feat / 4 floats apart
    return "windows", n * M                                                      # ed_launch_fnet_windows, two strides


def tiles(kind, total, M, B):
    """[(u0, nu)] of the launch and, per tile, the (frame, microphone) of each utterance as the kernel steps them
    (fnet_windows_kernels.hip:24-29: one division for the tile's first utterance, then ++mi, wrapping into ++fi)."""
    out = []
    for u0 in range(0, total, B):
        nu = min(B, total - u0)
        if kind == "windows":
            fi, mi = u0 // M, u0 - (u0 // M) * M
            step = []
            for _ in range(nu):
                step.append((fi, mi))
                mi += 1
                if mi == M:
                    mi, fi = 0, fi + 1
        elif kind == "by_frame":
            step = [(u, 0) for u in range(u0, u0 + nu)]
        else:
            step = [(0, u) for u in range(u0, u0 + nu)]
        out.append((u0, nu, step))
    return out


# ---- the emulator ------------------------------------------------------------------------------------------------------------------
class _Buf:
    """One of the two sliding buffers of all microphones, `per` elements each plus the slack behind the last: kept for the watched
    microphones only, addressed as the device buffer is. A write to a microphone that is not kept is dropped, a read of one gives POISON."""

    def __init__(self, M, per, slack, watched):
        self.M, self.per = M, per
        self.mics = {m: np.full(per + (slack if m == M - 1 else 0), POISON, np.int64) for m in watched}

    def mic(self, m):
        return self.mics.get(m)

    def _pieces(self, at, n):
        assert at >= 0
        k = 0
        while k < n:
            m = min((at + k) // self.per, self.M - 1)
            off = at + k - m * self.per
            room = (self.per if m < self.M - 1 else (len(self.mics[m]) if m in self.mics else self.per + SLACK)) - off
            take = min(n - k, room)
            assert take > 0, "outside the buffer and its slack"
            yield m, off, k, take
            k += take

    def put(self, at, n, vals):
        for m, off, k, take in self._pieces(at, n):
            if m in self.mics:
                self.mics[m][off:off + take] = vals if np.isscalar(vals) else vals[k:k + take]

    def get(self, at, n):
        out = np.full(n, POISON, np.int64)
        for m, off, k, take in self._pieces(at, n):
            if m in self.mics:
                out[k:k + take] = self.mics[m][off:off + take]
        return out


def watched_mics(M):
    return list(range(M)) if M <= 64 else sorted({0, 1, 2, M - 3, M - 2, M - 1} | set(range(0, M, 97)))


def walk(row, n_cu=N_CU, shift=shift_rounds, hold=hold_rounds, variant=None, check=True):
    """Walks the row's push schedule through the float bank with buffers of tokens -- one per sample, one per BYTE of a feature row, as
    the core shifts and holds float rows by bytes. Returns (items, problems): the coverage items reached, and what a consumer would have
    read wrong (empty for the real rules). `variant` swaps one rule for a mis-reading: mic_major (outputs), fi_mi_swapped (the windows
    kernel's two strides), no_feat_skip (the host flow's rows of utterance u), pitch_in_floats (the firmware flow's copy), shared_state
    (one filter state), fill_present (the fill written to the present microphones). A microphone's tokens count the frames of its own
    stream, so a push it was absent from must leave no trace."""
    s, g, pl = sizes(row), GEOMS[row["geom"]][1], plan_of(row["net"], row["geom"])
    F, nm, hop, N, tail, M = s["F"], s["nm"], s["hop"], s["N"], s["tail"], s["n_mics"]
    A, FB, E = s["mic_audio"], s["mic_feat"], FEAT_ELEM
    n_out, B = pl["n_out"], pl["batch"]
    watched = watched_mics(M)
    wset = set(watched)
    audio, feat = _Buf(M, A, SLACK // 2, watched), _Buf(M, FB, SLACK, watched)
    epoch, cnt = [0] * M, [0] * M
    seen, pos, shifted = 0, 0, False
    items, problems = set(), []
    mic_rows = FB // E                            # edison_float_bank.hip:67

    def start_state(m):                           # start_state, edison_stream_core.hip:220-245, at the current pos
        epoch[m] += 1
        cnt[m] = 0
        if m in wset:
            audio.mic(m)[pos * hop:pos * hop + tail] = _tok(m, epoch[m], 0, 0) + np.arange(tail)
            feat.mic(m)[pos * nm * E:(pos + F - 1) * nm * E] = _tok(m, epoch[m], 1, 0) + np.arange((F - 1) * nm * E)

    for m in range(M):
        start_state(m)
    resets = dict()
    for at, who in row["resets"]:
        resets.setdefault(at, []).append(who)
    scale = float(geometry(row).net_input_scale)
    items |= {("slots", s["slots"], "single" if M == 1 else "bank"), ("tail", _band(tail)), ("feat_bytes", _band(s["feat_bytes"])),
              ("alpha", {0.0: "0", 1.0: "1"}.get(row["alpha"], "interior")), ("threshold", "tie" if row["thr"] == "tie" else "plain"),
              ("fsm", row["fsm"]), ("push", row["push"]), ("ref", row["ref"], "large" if M > 8 else "small"),
              ("flow", "q15" if row["q15"] else "host", "one" if M == 1 else "many"),
              ("clip", "default" if tuple(row["clip"]) == DEFAULT_CLIP else "narrow"), ("scale", "1" if scale == 1.0 else "other")}
    if n_out in (1, 6, 10):
        items.add(("n_out", n_out))
    items.add(("n_out", "256" if n_out == 256 else "above 128" if n_out > 128 else "a divisor of 256" if 256 % n_out == 0 else "no divisor of 256, below 128"))
    if row["push"] != "host":
        items.add(("outputs", row["outputs"]))    # a host push downloads every output

    fulls = 0
    for p, n in enumerate(row["sched"]):
        absent, reset_now = absent_of(row, p), set()
        gone = set(absent)
        masked = bool(row["present"]) and row["present"][p] is not None
        for who in resets.get(p, ()):
            will_shift = not (pos + n <= s["slots"] * s["chunk"] or pos == 0)
            if who == "all":                      # ed_stream_core_reset, edison_stream_core.hip:258-274
                pos = seen = 0
                for m in range(M):
                    start_state(m)
                items.add(("reset", "all"))
            else:
                start_state(who)
                reset_now.add(who)
                assert pos != 0
                items.add(("reset_mic", "first" if who == 0 else "last" if who == M - 1 else "inner"))
                items.add(("reset_mic", "right before a shift" if will_shift else "right after a shift" if shifted else "elsewhere"))
        assert 1 <= n <= s["chunk"]               # begin_push, :278
        host = row["push"] == "host" or (row["push"] == "alt" and n == s["chunk"] and fulls % 2 == 0)
        fulls += n == s["chunk"]
        # make_room, edison_stream_core.hip:131-140: f_src and feat_bytes in bytes of float rows
        if not (pos + n <= s["slots"] * s["chunk"] or pos == 0):
            a_src, f_src = pos * hop, pos * nm * E
            for what, src, count in (("samples", a_src, tail), ("rows", f_src, s["feat_bytes"])):
                if count:
                    items.add(("shift", what, "single" if M == 1 else "bank", "overlapping" if src < count else "touching" if src == count else "disjoint"))
                    if src < count:
                        items.add(("overlap", what, _band(count)))
            for m in watched:
                shift(audio.mic(m), a_src, tail)
                shift(feat.mic(m), f_src, s["feat_bytes"])
            pos, shifted = 0, True
        else:
            shifted = False
        # the upload, :281-287: a row of the copy per microphone, mic_audio samples apart
        for m in watched:
            at = pos * hop + tail
            assert at + n * hop <= A
            audio.mic(m)[at:at + n * hop] = GARBAGE if m in gone else _tok(m, epoch[m], 0, tail + cnt[m] * hop) + np.arange(n * hop)
        # ---- the feature rows of all n_mics * n frames, edison_float_bank.hip:68-94
        rows0 = (pos + F - 1) * nm                # `rows` of microphone 0, in floats
        group = 0 if M == 1 else A                # utt_stride / group_stride: an utterance of the launch = a microphone
        items.add(("mfcc", "frames_per_utt", "1" if n == 1 else "chunk" if n == s["chunk"] else "ragged"))

        def row_tokens(u, f0, k):
            return GARBAGE if u in gone else _tok(u, epoch[u], 1, (F - 1 + cnt[u] + f0) * nm * E) + np.arange(k * nm * E)

        def read_frame(u, f):
            x0 = pos * hop + u * group + f * hop
            assert u * A <= x0 and x0 + N <= (u + 1) * A, "frame outside its microphone's samples"
            if check and u in wset and u not in gone:
                if not np.array_equal(audio.get(x0, N), _tok(u, epoch[u], 0, (cnt[u] + f) * hop) + np.arange(N)):
                    problems.append(("samples", p, u, f))

        if row["q15"]:
            # variant C writes [n_mics][n][num_mfcc] compactly (one microphone: in place), :68-72; then ONE 2-D copy, a row of it a
            # microphone's n new rows, the destination's pitch mic_feat BYTES, :73-77
            qg = q15_grid(M * n, n_cu)
            items.add(("q15", "grid at its cap" if qg["capped"] else "grid below its cap"))
            for u in (range(M) if M <= 64 else watched):
                for f in range(n):
                    read_frame(u, f)
            pitch = FB // E if variant == "pitch_in_floats" else FB
            for m in range(M):
                at = rows0 * E + (m * pitch if M > 1 else 0)
                if variant is None:
                    assert m * FB <= at and at + n * nm * E <= (m + 1) * FB, "rows outside their microphone's"
                feat.put(at, n * nm * E, row_tokens(m, 0, n))
        else:
            # ONE ed_mfcc_geom_fnet_kernel launch, :81-88; frame gi is frame f of utterance u (mfcc_geom_frames.inc:19-22), its row
            # out[gi * n_coef + feat_skip * u] (mfcc_geom_fnet_kernels.hip:18-19), feat_utt_stride = mic_feat / 4 floats, one microphone: 0
            ml = mfcc_launch(g, M * n, n_cu)
            items |= {("mfcc", "team", ml["team"]), ("mfcc", "wraps" if ml["wraps"] else "one pass")}
            fus = 0 if M == 1 else mic_rows
            feat_skip = fus - n * nm if fus and variant != "no_feat_skip" else 0
            for gi in range(M * n):
                u, f = divmod(gi, n)
                if M > 64 and u not in wset and variant is None:
                    continue
                read_frame(u, f)
                o = rows0 + gi * nm + feat_skip * u
                if variant is None:
                    assert u * mic_rows <= o and o + nm <= (u + 1) * mic_rows, "row outside its microphone's rows"
                feat.put(o * E, nm * E, row_tokens(u, f, 1))
        # ---- the network, :91-96
        kind, total = net_launch(row, n)
        items.add(("net", kind))
        items.add(("tile", "under" if total < B else "equal" if total == B else "over ragged" if total % B else "over whole"))
        ts = tiles(kind, total, M, B)
        if len(ts) > 512:
            items.add(("tile", "more than 512 workgroups"))
        win0 = pos * nm
        entry = {}
        for u0, nu, step in ts:
            if kind == "windows" and step[0][0] != step[-1][0]:
                items.add(("tile", "straddles a frame"))
            for j, (fi, mi) in enumerate(step):
                U = u0 + j
                assert (fi, mi) == ((U // M, U % M) if kind == "windows" else (U, 0) if kind == "by_frame" else (0, U))
                if mi not in wset:
                    continue
                if kind == "windows" and variant == "fi_mi_swapped":
                    at = win0 + fi * mic_rows + mi * nm
                else:
                    at = win0 + mi * mic_rows + fi * nm          # in + mi * mic_stride + fi * frame_stride
                entry[U] = (mi, fi)
                if at * E + F * nm * E > M * FB + SLACK:
                    assert variant is not None, "window outside the rows and their slack"
                    problems.append(("window", p, mi, fi))
                    continue
                if variant is None:
                    assert mi * FB <= at * E and (at + F * nm) * E <= (mi + 1) * FB, "window outside its microphone's rows"
                if check and mi not in gone:
                    want = _tok(mi, epoch[mi], 1, (cnt[mi] + fi) * nm * E) + np.arange(F * nm * E)
                    if not np.array_equal(feat.get(at * E, F * nm * E), want):
                        problems.append(("window", p, mi, fi))
        # ---- the filter reads probs: the caller's where given, else the bank's own block (:193; a host push: always the block, :216)
        items.add(("probs", "the block, host push" if host else "the caller's" if row["outputs"] in ("all", "no_logits") else "the block, device push"))
        items.add(("masked filter" if masked else "filter", "n", "1" if n == 1 else ">256" if n > 256 else "ragged" if n < s["chunk"] else "chunk"))
        if n > 1 and M > 1:
            for m in watched:
                if variant == "shared_state" and m != 0:     # state[t] for state[m * n_out + t], edison_stream_core.hip:77
                    problems.append(("state", p, m))
                for i in range(n):
                    if entry.get(m * n + i if variant == "mic_major" else bs.out_index(i, m, M)) != (m, i):
                        problems.append(("filter", p, m, i))
                        break
        elif variant == "shared_state" and M > 1:
            problems.append(("state", p, 1))
        if masked:
            hold_and_fill(s, n_out, n_out * E, E, audio.mic, feat.mic, pos, n, absent, items, problems, p, hold, variant, shifted, reset_now)
        pos += n
        seen += n
        for m in range(M):
            cnt[m] += 0 if m in gone else n
    return items, problems


def is_overlap_row(row):
    return any(it[0] == "shift" and it[3] == "overlapping" for it in walk(row, check=False)[0])


def is_hold_overlap_row(row):
    return any(it[0] == "hold" and it[2] == "overlapping" for it in walk(row, check=False)[0])


def full_set():
    """Every item a row could reach."""
    s = {("slots", n, k) for n in (1, 8) for k in ("single", "bank")}
    s |= {(k, b) for k in ("tail", "feat_bytes") for b in ("0", "<256", ">256", "x256")}
    s |= {("alpha", a) for a in ("0", "1", "interior")} | {("threshold", "tie"), ("threshold", "plain"), ("fsm", True), ("fsm", False)}
    s |= {("push", p) for p in ("dev", "host", "alt")} | {("ref", "independent", "large"), ("ref", "independent", "small"), ("ref", "streams", "small")}
    s |= {("reset", "all")} | {("reset_mic", v) for v in ("first", "last", "inner", "right before a shift", "right after a shift", "elsewhere")}
    s |= {("shift", w, "bank", k) for w in ("samples", "rows") for k in ("overlapping", "touching", "disjoint")}
    s |= {("shift", w, "single", k) for w in ("samples", "rows") for k in ("overlapping", "disjoint")}
    s |= {("overlap", "samples", ">256"), ("overlap", "rows", ">256"), ("overlap", "rows", "x256")}
    s |= {("mfcc", "team", 64), ("mfcc", "team", bs.EDG_BLOCK), ("mfcc", "wraps"), ("mfcc", "one pass")} | {("mfcc", "frames_per_utt", v) for v in ("1", "ragged", "chunk")}
    s |= {("filter", "n", v) for v in ("1", "ragged", ">256", "chunk")} | {("masked filter", "n", v) for v in ("1", "ragged", ">256", "chunk")}
    s |= {("flow", f, k) for f in ("host", "q15") for k in ("one", "many")} | {("q15", "grid at its cap"), ("q15", "grid below its cap")}
    s |= {("net", k) for k in ("by_frame", "by_microphone", "windows")}
    s |= {("tile", v) for v in ("under", "equal", "over ragged", "over whole", "straddles a frame", "more than 512 workgroups")}
    s |= {("n_out", v) for v in (1, 6, 10, "above 128", "no divisor of 256, below 128", "a divisor of 256", "256", "above 256")}
    s |= {("clip", "default"), ("clip", "narrow"), ("scale", "1"), ("scale", "other")}
    s |= {("outputs", o) for o in ("all", "no_probs", "no_logits", "none")}
    s |= {("probs", v) for v in ("the caller's", "the block, host push", "the block, device push")}
    s |= {("n_mics", ">4096"), ("n_mics x chunk", ">=2^31"), ("flow", "q15", "a sample history")}
    return s | bs.mask_set()


# item -> the host check or launch rule that keeps every accepted bank from it
EXCLUDED = {
    ("n_mics", ">4096"): "edison_float_bank.hip:152 refuses n_mics outside 1 .. 4096 (tests/test_gpu_float_bank.py::test_errors runs it)",
    ("n_mics x chunk", ">=2^31"): "edison_float_bank.hip:170 refuses it",
    ("n_out", "above 256"): "edison_float_bank.hip:166 refuses the filter for a network of more than 256 outputs, and every row filters",
    ("flow", "q15", "a sample history"): "edison_fnet.hip:310 admits the firmware flow at frame_len = frame_step = 1024 only, so tail = 0 "
                                         "(edison_stream_core.hip:159) and its banks never shift or hold samples",
}
