"""The fast MFCC loop's sweep: named calls chosen so that together they launch every instance ed_mfcc2_body (csrc/mfcc_kernels.hip) is
compiled to, at every shape of its work split.

Test infrastructure, not a test: tests/test_mfcc_sweep_cpu.py checks that the rows reach all 28 instances, that each note names the
instance the restated launch code (instance() below) gives its row, that the filterbanks have the table properties they are here for and
that the frame counts hit every case of the restated work split (split() below); tests/test_gpu_mfcc_sweep.py runs every row on the GPU.

The loop is compiled 28 times:
    {mfcc2, window, flag} x {ALIGNED, not} x {PLAIN, grouped} x {2+5, 3+6}   = 24    (ed_mfcc2_kernel, _window_kernel, _flag_kernel)
    list x {ALIGNED, not} x {2+5, 3+6}                                       =  4    (ed_mfcc2_list_kernel: never PLAIN)
An instance is (kernel, aligned, plain, shape).

A row is a dict:
  entry       Context method: mfcc / mfcc_rows / kws stage host arrays into a fresh (4-byte aligned) device buffer, the *_t ones take
              device tensors at the address given
  variant     "A" | "B" | "TF";  log: variant B's optional logarithm
  bank        a name of FILTERBANKS
  off         device entries: the audio is a view that starts `off` samples into a larger allocation (odd: 2-byte aligned only);
              mfcc_batches_t: one offset per batch
  hop         frame_step; never below 1024 here, so that every frame is one whole frame of the 64-frame base set
  group       None (one flat batch) or (frames_per_group, pad): group g starts at g * ((fpg - 1) * hop + 1024 + pad) samples; for
              kws rows fpg is 31 and hop 1024 (utt_stride = 31744 + pad); n_utt == 1 makes such a call PLAIN
  n_coef, feat_scale, outs ("f" float32, "q" int8, "fq" both);  big: the row also runs the largest counts
  note        "<kernel> <aligned|unaligned> <plain|grouped> <shape>; why"
"""
import os
import re

import lds_layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edison_amd", "csrc")
FRAME = 1024
UTT_FRAMES = 31
N_BASE = 64                      # distinct frames of the base set
LIST_BATCHES = 3                 # batches of a mfcc_batches_t row (one launch holds up to 16)
CU_LDS_BYTES = 160 * 1024        # LDS of one gfx950 CU
VARIANT_CODE = {"A": 0, "B": 1, "TF": 3}     # _lib.MFCC_A / MFCC_B / MFCC_TF

KERNELS = ("mfcc2", "window", "flag", "list")
SHAPES = ("2+5", "3+6")

# name -> (sample_rate, lower_edge_hertz, upper_edge_hertz, EDISON_FORCE_WIDE_MEL) and what the bank is here for
# (tests/test_mfcc_sweep_cpu.py reads the properties back from ed_build_mfcc_tables). A native 3+6 table uses the third narrow quad
# when a band below 16 spans 9 or more spectrum quads and the sixth wide quad when a band from 16 up spans 21 or more; on a mel scale
# 32 bands over 513 bins cannot do both (the bands would have to be about 31 and 79 bins wide at numbers 15 and 31: over 600 bins in
# all), so the two last quads come from two banks: a nearly linear one (all edges far below 700 Hz) and a strongly curved one.
FILTERBANKS = {
    "shipped": (16000.0, 80.0, 7600.0, False),            # needs 2+5
    "shipped_forced": (16000.0, 80.0, 7600.0, True),      # the same weights in the 3+6 table: the extra quads carry +0.0
    "wide6": (32000.0, 0.0, 16000.0, False),              # needs 3+6; non-zero weights in quad 5 of the wide part
    "narrow3": (500.0, 0.0, 250.0, False),                # needs 3+6; non-zero weights in quad 2 of the narrow part
}
BANK_CLAIMS = {
    "shipped": dict(shape="2+5", native=True),
    "shipped_forced": dict(shape="3+6", native=False),
    "wide6": dict(shape="3+6", native=True, last_wide_quad=True),
    "narrow3": dict(shape="3+6", native=True, last_narrow_quad=True),
}


# ---- the launch code, restated ---------------------------------------------------------------------------------------------------
def ed2_wpb():
    """ED2_WPB of the product build, from the source as lds_layout.layout_constants() reads its constants"""
    text = open(os.path.join(CSRC, "mfcc_kernels.hip")).read()
    return int(re.search(r"#ifndef ED2_WPB\s*\n#define ED2_WPB (\d+)", text).group(1))


def _fixtab_floats():
    text = open(os.path.join(CSRC, "mfcc_one_frame.h")).read()
    expr = re.search(r"#define ED_FIXTAB_FLOATS \(([0-9+* ]+)\)", text).group(1)
    return eval(expr, {"__builtins__": {}})


def lds_bytes(shape):
    """lds2 of ed_launch_mfcc_shape / _list_shape / _flag_shape: tables + (NLO + NHI) x 64 weight quads + a buffer per wave + the queue"""
    nlo, nhi = (int(v) for v in shape.split("+"))
    return 4 * (_fixtab_floats() + (nlo + nhi) * 256 + ed2_wpb() * L.layout_constants()["ED2_XBUF_FLOATS"]) + 16


def blocks_per_cu(shape):
    """What the occupancy query of ed_kernel_prepare answers for the loop: LDS is what limits it (64 * ED2_WPB threads, 160 VGPRs)"""
    return CU_LDS_BYTES // lds_bytes(shape)


def split(n_frames, n_cu, blocks_per_cu=1):
    """[(s0, cnt)] per workgroup: the slices of the frame pairs (ed_mfcc2_body; grid as the three launch functions size it)"""
    w = ed2_wpb()
    n_pairs = (n_frames + 1) // 2
    grid = min((n_pairs + w - 1) // w, n_cu * blocks_per_cu)
    return [(b * n_pairs // grid, (b + 1) * n_pairs // grid - b * n_pairs // grid) for b in range(grid)]


def cases(n_frames, n_cu, blocks_per_cu=1):
    """What a frame count does to the split, as tags"""
    w, s = ed2_wpb(), split(n_frames, n_cu, blocks_per_cu)
    cnts, full = [c for _, c in s], len(s) == n_cu * blocks_per_cu
    out = set()
    if len(s) == 1 and cnts[0] <= w:
        out.add("one workgroup, nothing drawn")                       # every pair is some wave's first pair
    if len(s) > 1 and min(cnts) < w:
        out.add("waves start without a pair")
    if full and min(cnts) < w:
        out.add("full grid, a short slice")
    if full and set(cnts) == {w}:
        out.add("full grid, every slice exactly one pair per wave")
    if full and set(cnts) == {w, w + 1}:
        out.add("full grid, slices of one pair per wave and one more")
    if cnts[-1] > w:
        out.add("last pair drawn, " + ("no frame B" if n_frames % 2 else "with frame B"))
    if min(cnts) >= 4 * w:
        out.add("several passes")
    if n_frames % 2:
        out.add("odd")
    return out


def FRAME_COUNTS(n_cu, blocks_per_cu=1):
    """The frame counts of the sweep for a device of n_cu compute units (see cases())"""
    w, g = ed2_wpb(), n_cu * blocks_per_cu
    full = 2 * w * g
    return sorted({1, 2, 3, 2 * w - 1, 2 * w, 2 * w + 1, full - 3, full - 1, full, full + 1, full + 2, 5 * full + 7, 65535})


def instance(call):
    """(kernel, aligned, plain, shape) of a call, as ed_launch_mfcc_shape, ed_launch_mfcc_list_shape and ed_launch_mfcc_flag_shape pick
    it. call: entry, ptr (the audio's device address; mfcc_batches_t: ptrs, one per batch), hop, fpg, group_stride, n_frames, window,
    exact, shape (mel_NLO + mel_NHI of the context's tables)."""
    if call["entry"] == "mfcc_batches_t":
        aligned = call["hop"] % 2 == 0 and all(p % 4 == 0 for p in call["ptrs"])
        return ("list", aligned, False, call["shape"])
    aligned = call["ptr"] % 4 == 0 and call["hop"] % 2 == 0 and call["group_stride"] % 2 == 0
    plain = call["fpg"] >= call["n_frames"]
    kernel = "flag" if call["exact"] else ("window" if call["window"] else "mfcc2")
    return (kernel, aligned, plain, call["shape"])


def all_instances():
    out = {(k, a, p, s) for k in KERNELS[:3] for a in (True, False) for p in (True, False) for s in SHAPES}
    return out | {("list", a, False, s) for a in (True, False) for s in SHAPES}


# instance -> the line of an entry point that refuses every call that would select it. None: exact mode works behind
# edison_mfcc_configure (the float64 tables of all three extra banks fit ED_EXACT_TAPS_MAX) and one utterance makes it PLAIN.
EXCLUDED = {}


# ---- the rows --------------------------------------------------------------------------------------------------------------------
HOST_ENTRIES = ("mfcc", "mfcc_rows", "kws")
ROWS = {}


def _row(name, entry, variant, bank, note, log=False, off=0, hop=FRAME, group=None, n_coef=13, feat_scale=1.0, outs="f", big=False, n_utt_one=False):
    assert entry not in HOST_ENTRIES or off == 0, "a host array is staged into a fresh allocation: its own address does not reach the kernel"
    ROWS[name] = dict(name=name, entry=entry, variant=variant, bank=bank, log=log, off=off, hop=hop, group=group, n_coef=n_coef,
                      feat_scale=feat_scale, outs=outs, big=big, n_utt_one=n_utt_one, note=note)


S3 = 0.3          # a feat_scale that is no power of two
# ed_mfcc2_kernel
_row("flat_A", "mfcc_t", "A", "shipped", "mfcc2 aligned plain 2+5; the benchmark's call, every count", outs="fq", big=True)
_row("flat_Blog_oddbase", "mfcc_t", "B", "shipped", "mfcc2 unaligned plain 2+5; a view from an odd sample; log on B at every count",
     log=True, off=1, n_coef=32, outs="fq", feat_scale=0.5)
_row("rows_B", "mfcc_rows_t", "B", "shipped", "mfcc2 aligned grouped 2+5; rows of 3 frames: every other pair straddles two rows",
     group=(3, 6), n_coef=31, outs="fq", feat_scale=S3)
_row("rows_A_oddstride", "mfcc_rows", "A", "shipped", "mfcc2 unaligned grouped 2+5; an odd row stride through the host entry point",
     group=(3, 7), n_coef=32)
_row("flat_B_wide6", "mfcc_t", "B", "wide6", "mfcc2 aligned plain 3+6; weights in the sixth wide quad", n_coef=1, outs="fq", feat_scale=S3)
_row("flat_A_narrow3_oddhop", "mfcc", "A", "narrow3", "mfcc2 unaligned plain 3+6; weights in the third narrow quad, an odd hop through the host entry point",
     hop=1025, n_coef=32, outs="fq")
_row("rows_A_forced", "mfcc_rows_t", "A", "shipped_forced", "mfcc2 aligned grouped 3+6; the shipped weights in the wide table", group=(3, 2), outs="q", feat_scale=0.5)
_row("rows_Blog_narrow3_oddstride", "mfcc_rows_t", "B", "narrow3", "mfcc2 unaligned grouped 3+6; odd row stride", log=True, group=(3, 1), n_coef=31)
# ed_mfcc2_window_kernel
_row("tf_flat", "mfcc_t", "TF", "shipped", "window aligned plain 2+5; every count, int8 features", outs="fq", big=True)
_row("tf_oddhop", "mfcc_t", "TF", "shipped", "window unaligned plain 2+5; odd hop", hop=1027, n_coef=32, outs="fq", feat_scale=S3)
_row("tf_rows", "mfcc_rows_t", "TF", "shipped", "window aligned grouped 2+5; int8 features only", group=(3, 10), outs="q")
_row("tf_rows_oddbase", "mfcc_rows_t", "TF", "shipped", "window unaligned grouped 2+5; odd base, even stride", off=3, group=(3, 4), n_coef=31)
_row("tf_flat_narrow3", "mfcc_t", "TF", "narrow3", "window aligned plain 3+6; third narrow quad", n_coef=32)
_row("tf_oddbase_wide6", "mfcc_t", "TF", "wide6", "window unaligned plain 3+6; sixth wide quad", off=1, n_coef=1)
_row("tf_rows_wide6", "mfcc_rows_t", "TF", "wide6", "window aligned grouped 3+6", group=(3, 0), n_coef=32, outs="fq", feat_scale=0.5)
_row("tf_rows_forced_oddstride", "mfcc_rows_t", "TF", "shipped_forced", "window unaligned grouped 3+6; odd stride", group=(3, 9), outs="fq", feat_scale=S3)
# ed_mfcc2_flag_kernel (exact KWS mode: 31 frames per utterance, hop 1024, 13 coefficients, int8 only)
_row("exact_one", "kws_t", "B", "shipped", "flag aligned plain 2+5; one utterance: 16 pairs in two workgroups", group=(31, 256), outs="q", n_utt_one=True)
_row("exact_one_oddbase", "kws_t", "B", "shipped", "flag unaligned plain 2+5; one utterance from an odd sample", off=1, group=(31, 256), outs="q", n_utt_one=True)
_row("exact_many", "kws_t", "B", "shipped", "flag aligned grouped 2+5; stride 32000, every count", group=(31, 256), outs="q", big=True)
_row("exact_many_oddstride", "kws", "B", "shipped", "flag unaligned grouped 2+5; odd utterance stride through the host entry point", group=(31, 1), outs="q")
_row("exact_one_wide6", "kws_t", "B", "wide6", "flag aligned plain 3+6; a reconfigured filterbank", group=(31, 0), outs="q", n_utt_one=True)
_row("exact_one_narrow3_oddstride", "kws", "B", "narrow3", "flag unaligned plain 3+6; one utterance with an odd stride", group=(31, 5), outs="q", n_utt_one=True)
_row("exact_many_forced", "kws_t", "B", "shipped_forced", "flag aligned grouped 3+6; stride 31744", group=(31, 0), outs="q")
_row("exact_many_narrow3_oddbase", "kws_t", "B", "narrow3", "flag unaligned grouped 3+6; odd base", off=1, group=(31, 256), outs="q")
# ed_mfcc2_list_kernel
_row("list_A", "mfcc_batches_t", "A", "shipped", "list aligned grouped 2+5; three batches, every count", off=(0, 0, 0), outs="fq", big=True)
_row("list_Blog_oddptr", "mfcc_batches_t", "B", "shipped", "list unaligned grouped 2+5; the middle batch starts at an odd sample", log=True, off=(0, 1, 0), n_coef=32,
     outs="fq", feat_scale=S3)
_row("list_B_wide6", "mfcc_batches_t", "B", "wide6", "list aligned grouped 3+6", off=(2, 0, 4), n_coef=31)
_row("list_A_narrow3_oddhop", "mfcc_batches_t", "A", "narrow3", "list unaligned grouped 3+6; odd hop", off=(0, 0, 0), hop=1025, n_coef=1, outs="fq", feat_scale=0.5)


def is_kws(row):
    return row["entry"] in ("kws", "kws_t")


def unit(row):
    """Frames come in whole rows / utterances / equal batches: the row's frame counts are multiples of this"""
    if row["entry"] == "mfcc_batches_t":
        return LIST_BATCHES
    return row["group"][0] if row["group"] else 1


def geometry(row, n_frames):
    """(frames_per_group, group_stride) as the entry point hands them to the launch; for the list: per batch"""
    if row["entry"] == "mfcc_batches_t":
        return n_frames // LIST_BATCHES, 0
    if row["group"] is None:
        return n_frames, 0
    fpg, pad = row["group"]
    return fpg, (fpg - 1) * row["hop"] + FRAME + pad


def row_counts(row, n_cu):
    """The frame counts row `row` runs: FRAME_COUNTS(n_cu) (up to one full grid and two frames unless the row is `big`), each replaced by
    the nearest multiples of unit(row) below and above it where the entry point takes whole rows, utterances or equal batches; a
    grouped row never runs less than two groups (one group is the PLAIN instance). A one-utterance row has 31 frames and nothing else."""
    u, w = unit(row), ed2_wpb()
    if row["n_utt_one"]:
        return [UTT_FRAMES]
    lo = 2 * u if row["group"] else u
    out = set()
    for c in FRAME_COUNTS(n_cu, blocks_per_cu(SHAPES[0])):
        if not row["big"] and c > 2 * w * n_cu + 2:
            continue
        out |= {max(m, lo) for m in (c // u * u, -(-c // u) * u)}
    return sorted(out)


def call(row, n_frames, shape):
    """The call of row `row` at n_frames frames as instance() wants it; device addresses relative to a 4-byte aligned allocation"""
    fpg, gs = geometry(row, n_frames)
    d = dict(entry=row["entry"], hop=row["hop"], fpg=fpg, group_stride=gs, n_frames=n_frames, window=row["variant"] == "TF",
             exact=is_kws(row), shape=shape)
    if row["entry"] == "mfcc_batches_t":
        d["ptrs"] = [2 * o for o in row["off"]]
    else:
        d["ptr"] = 2 * row["off"]
    return d


def bank_shape(lib, bank, variant):
    fs, lo, hi, force = FILTERBANKS[bank]
    t = L.build_tables(lib, VARIANT_CODE[variant], force, fs, lo, hi)
    return "%d+%d" % (t[5], t[6])


def note_instance(note):
    k, a, p, s = note.split(";")[0].split()
    assert a in ("aligned", "unaligned") and p in ("plain", "grouped"), note
    return (k, a == "aligned", p == "plain", s)


def row_items(lib, row, n_cu=256):
    """What row `row` is there for: the instance of every count it runs (one and the same), its bank, its entry point, its int8 scale"""
    shape = bank_shape(lib, row["bank"], row["variant"])
    inst = {instance(call(row, n, shape)) for n in row_counts(row, n_cu)}
    out = {("instance",) + i for i in inst} | {("bank", row["bank"]), ("entry", row["entry"])}
    if "q" in row["outs"] and not is_kws(row):
        out.add(("feat_scale", row["feat_scale"]))
    if row["log"]:
        out.add(("log", row["entry"]))
    return out


def full_items():
    out = {("instance",) + i for i in all_instances()} | {("bank", b) for b in FILTERBANKS}
    out |= {("entry", e) for e in ("mfcc", "mfcc_t", "mfcc_rows", "mfcc_rows_t", "mfcc_batches_t", "kws", "kws_t")}
    return out | {("feat_scale", s) for s in (1.0, 0.5, S3)}


# ---- addressing forms for the comparison across instances: one variant, one table, the same 66 frames -------------------------------
# name -> (entry, off, hop, group); TF has no list entry point
FORMS = {
    "flat": ("mfcc_t", 0, FRAME, None),
    "flat odd base": ("mfcc_t", 1, FRAME, None),
    "flat odd hop": ("mfcc_t", 0, 1025, None),
    "rows": ("mfcc_rows_t", 0, FRAME, (3, 6)),
    "rows odd stride": ("mfcc_rows_t", 0, FRAME, (3, 7)),
    "rows odd base": ("mfcc_rows_t", 1, FRAME, (3, 6)),
    "rows of 1, odd stride": ("mfcc_rows_t", 0, FRAME, (1, 1)),
    "list": ("mfcc_batches_t", (0, 0, 0), FRAME, None),
    "list odd pointer": ("mfcc_batches_t", (0, 0, 1), FRAME, None),
    "list odd hop": ("mfcc_batches_t", (0, 0, 0), 1027, None),
}


def form_row(form, variant, log, bank):
    entry, off, hop, group = FORMS[form]
    return dict(name=form, entry=entry, variant=variant, bank=bank, log=log, off=off, hop=hop, group=group, n_coef=32, feat_scale=1.0, outs="f",
                big=False, n_utt_one=False, note="")
