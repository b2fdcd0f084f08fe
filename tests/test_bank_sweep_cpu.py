"""The stream-bank sweep without a GPU: the rows of tests/bank_sweep.py reach every item of the restated push (bank_sweep.walk) but
those in bank_sweep.EXCLUDED, each row is needed for at least one of them, every row passes the create checks, the restated buffer
sizes are the ones edison_stream_core.h computes, and every row's push schedule walks through the emulator of the core -- numpy
buffers of opaque tokens, the shift in the kernels' rounds of 256 -- with every frame the MFCC reads and every window the network reads
holding exactly that microphone's newest samples and rows, inside its buffers. The same walk with the shift's waves left unordered goes
wrong on exactly the rows whose shift overlaps, and with one indexing rule swapped for a mis-reading on every row that can tell. Rows
with masks add the hold of the absent microphones and the filter kernel's fill; the hold with its rounds from the bottom up goes wrong
on exactly the rows whose hold overlaps."""
import functools
import os
import subprocess

import pytest

import bank_sweep as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _walk(name):
    return bs.walk(bs.ROWS[name])


def _missing(names):
    have = set().union(*(_walk(n)[0] for n in names))
    return sorted(bs.full_set() - set(bs.EXCLUDED) - have, key=str)


def test_the_rows_cover_every_item(built_lib):
    assert _missing(bs.ROWS) == [], "items no row reaches"
    reached = set().union(*(_walk(n)[0] for n in bs.ROWS))
    assert reached <= bs.full_set(), sorted(reached - bs.full_set(), key=str)
    # an exclusion is a reason that names the line which rules the item out, and no row reaches what it excludes
    assert set(bs.EXCLUDED) <= bs.full_set() and not set(bs.EXCLUDED) & reached
    assert all(isinstance(v, str) and ".hip:" in v for v in bs.EXCLUDED.values())
    # the row that runs one launch past the general kernel's grid cap does so by one input
    assert bs.ROWS["gen_cap"]["n_mics"] == 1 and bs.ROWS["gen_cap"]["chunk"] == bs.general_cap(bs.N_CU) + 1


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_every_row_is_needed(built_lib, name):
    assert _missing([n for n in bs.ROWS if n != name]) != [], "row %s reaches nothing the others do not" % name


def test_every_row_passes_the_create_checks_and_the_excluded_sizes_do_not(built_lib):
    for name, row in bs.ROWS.items():
        assert bs.create_check(row) is None, (name, bs.create_check(row))
    one = bs.ROWS["fast_3"]
    assert "n_mics" in bs.create_check(dict(one, n_mics=bs.MAX_MICS + 1)) and "n_mics" in bs.create_check(dict(one, n_mics=0))
    assert "2^30" in bs.create_check(dict(one, chunk=1 << 20))
    # 4096 microphones x 2^19 frames of 64 samples pass every other check and are refused for their 2^31 frames per push
    assert "2^31" in bs.create_check(dict(bs.ROWS["odd_ov"], n_mics=4096, chunk=1 << 19))
    # the overlap geometries: frame_len > 9 x frame_step; the one-slot geometry: the smallest chunk past 4 Mi samples
    for g in ("square_ov", "shipped_ov256", "odd_ov"):
        assert bs.GEOMS[g][1]["frame_len"] > 9 * bs.GEOMS[g][1]["frame_step"]
    step = bs.GEOMS["shipped_slot1"][1]["frame_step"]
    assert (bs.SLOT1_CHUNK - 1) * step * 2 * 8 <= 64 << 20 < bs.SLOT1_CHUNK * step * 2 * 8 and bs.SLOT1_CHUNK * step > 4 << 20


PROBE = r"""
#include <stdio.h>
#include "edison_stream_core.h"
int main(void)
{
	int k[6];
	while (scanf("%d %d %d %d %d %d", k, k + 1, k + 2, k + 3, k + 4, k + 5) == 6)
	{
		const size_t push = (size_t)k[2] * k[3];
		const int slots = push * sizeof(int16_t) * ED_STREAM_CORE_SLOTS <= ED_STREAM_CORE_SLOTS_BYTES ? ED_STREAM_CORE_SLOTS : 1;
		printf("%d %zu %zu %d %zu\n", slots, ed_stream_core_mic_audio(k[0], slots, k[2], k[3]), ed_stream_core_mic_feat(1, k[4], slots, k[2], k[5]),
		       ED_STREAM_CORE_SLACK, ed_stream_core_align((size_t)k[0]));
	}
	return 0;
}
"""


def test_restated_sizes_equal_the_headers(built_lib, tmp_path):
    """edison_stream_core.h compiles on the host: its own mic_audio, mic_feat, slack and the 64 MB rule's constants for every row."""
    from edison_amd import build as B
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    rocm = os.path.dirname(os.path.dirname(B._hipcc()))
    inc = ["-D__HIP_PLATFORM_AMD__", "-I" + B.CSRC, "-I" + os.path.join(ROOT, "include")]
    r = subprocess.run(["g++", "-std=c++17"] + inc + ["-I" + os.path.join(rocm, "include"), str(src), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([B._hipcc(), "-std=c++17", "-x", "c++"] + inc + [str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes = [bs.sizes(row) for row in bs.ROWS.values()]
    text = "".join("%d %d %d %d %d %d\n" % (s["tail"], 0, s["chunk"], s["hop"], s["F"], s["nm"]) for s in sizes)
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(lines) == len(sizes)
    for s, ln in zip(sizes, lines):
        slots, audio, feat, slack, al = (int(v) for v in ln.split())
        assert (slots, audio, feat, slack) == (s["slots"], s["mic_audio"], s["mic_feat"], bs.SLACK), s
        assert al == -(-s["tail"] // 16) * 16


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_the_walk_reads_what_each_microphone_pushed(built_lib, name):
    """No problems under the real rules; the position sequence ends where frames_seen says."""
    items, problems = _walk(name)
    assert problems == [], problems[:5]
    row = bs.ROWS[name]
    assert bs.is_overlap_row(row) == any(it[0] == "shift" and it[3] == "overlapping" for it in items)
    if row["route"] == "fast" and row["n_mics"] >= 16:
        assert {it[1] for it in items if it[0] == "residue"} == set(range(16)), name


@pytest.mark.parametrize("name", list(bs.ROWS))
def test_unordered_waves_go_wrong_on_exactly_the_overlap_rows(built_lib, name):
    """The rounds exist for the overlap: without them (bank_sweep.shift_unordered) the walk reads wrong samples or rows on every row
    whose shift overlaps and on no other. An ascending copy in pieces of 64 (one wavefront) is right everywhere: the destination lies
    below the source."""
    row = bs.ROWS[name]
    bad = bs.walk(row, shift=bs.shift_unordered)[1]
    assert bool(bad) == bs.is_overlap_row(row), (name, bad[:3])
    assert bs.walk(row, shift=bs.shift_forward64)[1] == []


def test_there_are_overlap_rows_for_samples_and_rows_single_and_bank(built_lib):
    over = [n for n in bs.ROWS if bs.is_overlap_row(bs.ROWS[n])]
    assert {"square_ov", "shipped_ov256", "odd_ov"} <= set(over)
    for n in ("square_ov", "shipped_ov256", "odd_ov"):
        kinds = {p[0] for p in bs.walk(bs.ROWS[n], shift=bs.shift_unordered)[1]}
        assert kinds == {"samples", "window"}, (n, kinds)    # both buffers are caught


@pytest.mark.parametrize("variant", ["mic_major", "shared_state", "one_machine", "window_stride"])
def test_mis_readings_are_told_apart(built_lib, variant):
    """Mic-major outputs, state[t] for state[m * n_out + t], one machine for all microphones, a window stride one row off: each goes
    wrong on every row with several microphones (and several frames in a push, for the output order)."""
    for name, row in bs.ROWS.items():
        if row["n_mics"] > 64 or row["chunk"] > 300:
            continue        # the same rules at sizes where the walk is slow
        multi = row["n_mics"] > 1 and (variant == "window_stride" or max(row["sched"]) > 1)
        assert bool(bs.walk(row, variant=variant)[1]) == multi, (name, variant)
        if multi and variant != "window_stride":
            assert all(n != row["n_mics"] for n in row["sched"] if n > 1), name


MASKED = [n for n, r in bs.ROWS.items() if r["present"]]


def test_the_masked_rows_reach_every_item_of_a_masked_push(built_lib):
    """The hold over overlapping, touching and disjoint samples and rows, more than 256 bytes of rows to zero, the fill in one round,
    several and beyond 256 frames, 4096 workgroups: all from rows with masks, which are in the sweep for nothing else."""
    reached = set().union(*(_walk(n)[0] for n in MASKED))
    assert bs.mask_set() <= reached and all(it[0] in bs.MASKED_ROW_ITEMS for it in reached)
    assert not any(it in bs.mask_set() for n in bs.ROWS if n not in MASKED for it in _walk(n)[0])
    # 19 outputs: from 14 frames on the rows to zero pass 256 bytes and the fill its first round of 256 / 19 rows
    assert bs.graph_facts("even_same")["n_out"] == 19 and 13 * 19 <= 256 < 14 * 19


@pytest.mark.parametrize("name", MASKED)
def test_ascending_rounds_go_wrong_on_exactly_the_rows_whose_hold_overlaps(built_lib, name):
    """The hold moves the history UP, so its rounds run from the top down (edison_bank_hold.hip:22): from the bottom up a round's writes
    land on what a later round has yet to read, wherever the destination overlaps the source."""
    row = bs.ROWS[name]
    bad = bs.walk(row, hold=bs.hold_ascending)[1]
    assert bool(bad) == bs.is_hold_overlap_row(row), (name, bad[:3])
    assert {p[0] for p in bad} <= {"samples", "window"}


def test_the_fill_written_to_the_present_microphones_is_caught_on_every_masked_row(built_lib):
    for name, row in bs.ROWS.items():
        assert bool(bs.walk(row, variant="fill_present")[1]) == bool(row["present"]), name
    assert {n for n in MASKED if bs.is_hold_overlap_row(bs.ROWS[n])} == {"mask_even", "mask_touch", "mask_4096"}
