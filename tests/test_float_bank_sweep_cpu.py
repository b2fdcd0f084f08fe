"""The float-bank sweep without a GPU: the rows of tests/float_bank_sweep.py reach every item of the restated push
(float_bank_sweep.walk) but those in EXCLUDED, each row is needed for at least one of them, every row passes the create checks, the
restated buffer sizes with four-byte rows are the ones edison_stream_core.h computes, and every row's push schedule walks through the
emulator -- tokens per sample and per byte of a float row, the shift and the hold in the kernels' rounds of 256 -- with every frame the
feature launch reads and every window the network reads holding exactly that microphone's own stream, inside its buffers, whatever
pushes left it out. The shift with its waves left unordered goes wrong on exactly the rows whose shift overlaps, the hold with its rounds
from the bottom up on exactly the rows whose hold overlaps, and each indexing rule swapped for a mis-reading on every row that can tell."""
import functools
import os
import subprocess

import pytest

import bank_sweep as bs
import float_bank_sweep as fs
from test_bank_sweep_cpu import PROBE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _walk(name):
    return fs.walk(fs.ROWS[name])


def _missing(names):
    have = set().union(*(_walk(n)[0] for n in names))
    return sorted(fs.full_set() - set(fs.EXCLUDED) - have, key=str)


def test_the_rows_cover_every_item(built_lib):
    assert _missing(fs.ROWS) == [], "items no row reaches"
    reached = set().union(*(_walk(n)[0] for n in fs.ROWS))
    assert reached <= fs.full_set(), sorted(reached - fs.full_set(), key=str)
    assert set(fs.EXCLUDED) <= fs.full_set() and not set(fs.EXCLUDED) & reached
    assert all(isinstance(v, str) and ".hip:" in v for v in fs.EXCLUDED.values())
    assert bs.mask_set() <= reached


@pytest.mark.parametrize("name", list(fs.ROWS))
def test_every_row_is_needed(built_lib, name):
    assert _missing([n for n in fs.ROWS if n != name]) != [], "row %s reaches nothing the others do not" % name


def test_every_row_passes_the_create_checks_and_the_excluded_sizes_do_not(built_lib):
    for name, row in fs.ROWS.items():
        assert fs.create_check(row) is None, (name, fs.create_check(row))
    one = fs.ROWS["host_3x3"]
    assert "n_mics" in fs.create_check(dict(one, n_mics=fs.MAX_MICS + 1)) and "n_mics" in fs.create_check(dict(one, n_mics=0))
    assert "2^30" in fs.create_check(dict(one, chunk=1 << 22))
    assert "2^31" in fs.create_check(dict(fs.ROWS["ov_x256_5"], n_mics=4096, chunk=1 << 19))
    assert "clip" in fs.create_check(dict(one, clip=(1.0, -1.0)))
    # the firmware flow away from its framing; the state machine away from 10 classes
    assert "q15" in fs.create_check(dict(one, q15=True)) and "10 outputs" in fs.create_check(dict(one, fsm=True))
    for name, row in fs.ROWS.items():
        if row["q15"]:
            assert fs.sizes(row)["tail"] == 0, name
    # the overlap geometries: frame_len > 9 x frame_step; the one-slot geometry: the smallest chunk past 4 Mi samples
    for g in ("square_ov", "ov_x256"):
        assert fs.GEOMS[g][1]["frame_len"] > 9 * fs.GEOMS[g][1]["frame_step"]
    assert fs.sizes(fs.ROWS["ov_x256_5"])["feat_bytes"] % 256 == 0
    step = fs.GEOMS["shipped_slot1"][1]["frame_step"]
    assert (bs.SLOT1_CHUNK - 1) * step * 2 * 8 <= 64 << 20 < bs.SLOT1_CHUNK * step * 2 * 8


def test_restated_sizes_equal_the_headers(built_lib, tmp_path):
    """edison_stream_core.h compiles on the host: its own mic_audio, mic_feat at feat_elem = 4, slack and the 64 MB rule for every row."""
    from edison_amd import build as B
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE.replace("ed_stream_core_mic_feat(1,", "ed_stream_core_mic_feat(%d," % fs.FEAT_ELEM))
    assert "mic_feat(4," in src.read_text()
    exe = str(tmp_path / "probe")
    rocm = os.path.dirname(os.path.dirname(B._hipcc()))
    inc = ["-D__HIP_PLATFORM_AMD__", "-I" + B.CSRC, "-I" + os.path.join(ROOT, "include")]
    r = subprocess.run(["g++", "-std=c++17"] + inc + ["-I" + os.path.join(rocm, "include"), str(src), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([B._hipcc(), "-std=c++17", "-x", "c++"] + inc + [str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes = [fs.sizes(row) for row in fs.ROWS.values()]
    text = "".join("%d %d %d %d %d %d\n" % (s["tail"], 0, s["chunk"], s["hop"], s["F"], s["nm"]) for s in sizes)
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(lines) == len(sizes)
    for s, ln in zip(sizes, lines):
        slots, audio, feat, slack, _ = (int(v) for v in ln.split())
        assert (slots, audio, feat, slack) == (s["slots"], s["mic_audio"], s["mic_feat"], bs.SLACK), s
        assert s["feat_bytes"] == fs.FEAT_ELEM * (s["F"] - 1) * s["nm"] and s["mic_feat"] % fs.FEAT_ELEM == 0


@pytest.mark.parametrize("name", list(fs.ROWS))
def test_the_walk_reads_what_each_microphone_pushed(built_lib, name):
    """No problems under the real rules, and (the walk's own assertions) no read or write outside a microphone's buffers."""
    items, problems = _walk(name)
    assert problems == [], problems[:5]
    row = fs.ROWS[name]
    assert fs.is_overlap_row(row) == any(it[0] == "shift" and it[3] == "overlapping" for it in items)
    # the tiles are the network's own: 16 utterances, or what its LDS plan leaves
    assert 1 <= fs.plan_of(row["net"], row["geom"])["batch"] <= 16


@pytest.mark.parametrize("name", list(fs.ROWS))
def test_unordered_waves_go_wrong_on_exactly_the_overlap_rows(built_lib, name):
    row = fs.ROWS[name]
    bad = fs.walk(row, shift=fs.shift_unordered)[1]
    assert bool(bad) == fs.is_overlap_row(row), (name, bad[:3])
    assert fs.walk(row, shift=fs.shift_forward64)[1] == []


@pytest.mark.parametrize("name", [n for n, r in fs.ROWS.items() if r["present"]])
def test_ascending_rounds_go_wrong_on_exactly_the_rows_whose_hold_overlaps(built_lib, name):
    """The hold moves the history UP, so its rounds run from the top down (edison_bank_hold.hip:22): from the bottom up a round's writes
    land on what a later round has yet to read, wherever the destination overlaps the source."""
    row = fs.ROWS[name]
    bad = fs.walk(row, hold=fs.hold_ascending)[1]
    assert bool(bad) == fs.is_hold_overlap_row(row), (name, bad[:3])


def test_there_are_overlap_rows_for_the_shift_and_for_the_hold(built_lib):
    assert {"ov_single", "ov_x256_5", "host_17x2"} <= {n for n in fs.ROWS if fs.is_overlap_row(fs.ROWS[n])}
    for n in ("ov_single", "ov_x256_5"):
        assert {p[0] for p in fs.walk(fs.ROWS[n], shift=fs.shift_unordered)[1]} == {"samples", "window"}, n     # both buffers are caught
    assert {n for n, r in fs.ROWS.items() if r["present"] and fs.is_hold_overlap_row(r)} == {"filt_257", "mask_even", "mask_200", "mask_touch", "mask_4096"}
    assert {p[0] for p in fs.walk(fs.ROWS["mask_touch"], hold=fs.hold_ascending)[1]} == {"samples", "window"}
    assert {p[0] for p in fs.walk(fs.ROWS["mask_even"], hold=fs.hold_ascending)[1]} == {"window"}               # its samples move disjointly


def _can_tell(row, variant):
    """Whether the row's shapes tell the mis-reading from the rule."""
    multi, frames = row["n_mics"] > 1, max(row["sched"]) > 1
    return {"mic_major": multi and frames, "fi_mi_swapped": multi and frames, "no_feat_skip": multi and not row["q15"],
            "pitch_in_floats": multi and row["q15"], "shared_state": multi, "fill_present": bool(row["present"])}[variant]


@pytest.mark.parametrize("variant", ["mic_major", "fi_mi_swapped", "no_feat_skip", "pitch_in_floats", "shared_state", "fill_present"])
def test_mis_readings_are_told_apart(built_lib, variant):
    """Mic-major outputs, the windows kernel's two strides swapped, the host flow's rows without feat_skip, the firmware flow's copy with
    its pitch in floats, one filter state for all microphones, the fill written to the present microphones: each goes wrong on every
    row that can tell it from the rule, and on no other."""
    told = 0
    for name, row in fs.ROWS.items():
        if row["chunk"] > 300:
            continue        # the same rules at sizes where the walk is slow
        bad = fs.walk(row, variant=variant)[1]
        assert bool(bad) == _can_tell(row, variant), (name, variant, bad[:3])
        told += bool(bad)
    assert told >= 2, variant
