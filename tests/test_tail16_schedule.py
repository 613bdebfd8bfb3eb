"""tail16's static schedule (csrc/tail16_schedule.h), checked on the host: no GPU, no hipcc.

The header's constexpr functions are what the kernel calls; its static_asserts hold whenever it compiles.  Here
tools/tail16_schedule_print.cpp -- a stand-alone host program that includes the same header -- is built with the C++ compiler of
the machine and the table it prints is checked again from Python, independently of the header's own checking code:
  * every (100-level pixel, ConvT#3 tap row) column of a strip's 200 x 2 belongs to exactly one lane of one BC item; the merged
    item 12 holds pixels 192-199 with tap row 0 on lanes 0-7 and tap row 1 on lanes 8-15, lanes 16-31 nothing;
  * every D item 0-15 belongs to exactly one wave; role P (waves 0-7) has none; a pair is two consecutive items of a row pair, a
    wave's second pair has the j4 of its first and is not in row pair 0 (what the kernel's D code relies on);
  * per SIMD (wave % 4) the item counts are the ones DESIGN.md 4.1 states: 4 BC + 2 A on SIMD 0 (the SIMD with four BC items ends
    the round: no D item and not the merged item there), 3 BC + 2 A + 5 D on SIMDs 1 and 2, 3 BC + 2 A + 6 D on SIMD 3.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sr-for-cfd_amd", "csrc")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path_factory.mktemp("tail16_schedule") / "tail16_schedule_print"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tools", "tail16_schedule_print.cpp")],
                   check=True, capture_output=True, text=True)
    return json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)


def _d_items(w):
    items = []
    if w["d_count"] >= 1:
        items.append(w["d_first"])
    if w["d_count"] >= 2:
        items.append(w["d_first"] + 1)
    if w["d_count"] == 4:
        items += [w["d_second"], w["d_second"] + 1]
    return items


def test_shape_of_the_table(table):
    assert (table["waves"], table["simds"], table["role_p_waves"]) == (16, 4, 8)
    assert (table["bc_items"], table["a_items"], table["d_items"], table["bc_merged"]) == (13, 8, 16, 12)
    assert [w["wave"] for w in table["wave"]] == list(range(16))
    assert all(w["simd"] == w["wave"] % 4 for w in table["wave"])
    assert len(table["bc_lane"]) == 13 and all(len(lanes) == 32 for lanes in table["bc_lane"])


def test_every_bc_column_has_one_lane_of_one_item(table):
    owners = {}
    bc_waves = {}
    for w in table["wave"]:
        if w["bc"] < 0:
            continue
        assert 0 <= w["bc"] < 13
        assert w["bc"] not in bc_waves, "two waves run BC item %d" % w["bc"]
        bc_waves[w["bc"]] = w["wave"]
        for lane, (px, tap) in enumerate(table["bc_lane"][w["bc"]]):
            if px < 0:
                continue
            assert 0 <= px < 200 and tap in (0, 1), (w["bc"], lane, px, tap)
            owners.setdefault((px, tap), []).append((w["bc"], lane))
    assert sorted(bc_waves) == list(range(13))
    assert sorted(owners) == [(px, tap) for px in range(200) for tap in (0, 1)]
    assert all(len(v) == 1 for v in owners.values()), {k: v for k, v in owners.items() if len(v) != 1}


def test_merged_item_holds_both_tap_rows_of_pixels_192_to_199(table):
    lanes = table["bc_lane"][12]
    assert lanes[:8] == [[192 + l, 0] for l in range(8)]
    assert lanes[8:16] == [[192 + l, 1] for l in range(8)]
    assert all(px == -1 for px, _ in lanes[16:])
    for item in range(12):                       # one pixel tile and one tap row per item, 32 consecutive pixels
        assert table["bc_lane"][item] == [[32 * (item // 2) + l, item % 2] for l in range(32)]
    merged_wave = [w for w in table["wave"] if w["bc"] == 12]
    assert len(merged_wave) == 1 and merged_wave[0]["wave"] >= table["role_p_waves"], "the merged path exists in role Q's loop only"
    assert merged_wave[0]["simd"] != 0, "SIMD 0 carries four BC items: not the longest one too"


def test_every_d_item_has_one_wave_and_role_p_has_none(table):
    owners = {}
    for w in table["wave"]:
        assert w["d_count"] in (0, 1, 2, 4)
        for item in _d_items(w):
            owners.setdefault(item, []).append(w["wave"])
        if w["wave"] < table["role_p_waves"]:
            assert w["d_count"] == 0 and w["a"] == w["wave"]
        else:
            assert w["a"] == -1
    assert sorted(owners) == list(range(16))
    assert all(len(v) == 1 for v in owners.values()), owners


def test_d_pairs_are_what_the_d_code_can_run(table):
    for w in table["wave"]:
        if w["d_count"] >= 2:
            assert w["d_first"] % 2 == 0, w          # items 2k, 2k + 1: one row pair, neighbouring tile groups
        if w["d_count"] == 4:
            assert w["d_second"] % 2 == 0 and w["d_second"] % 4 == w["d_first"] % 4, w   # one set of lane offsets serves both pairs
            assert w["d_second"] // 4 != 0, w        # seams (row pair 0) go through d_first only
            assert w["d_second"] // 4 != w["d_first"] // 4, w


def test_per_simd_item_counts(table):
    per = {s: [0, 0, 0] for s in range(4)}
    for w in table["wave"]:
        per[w["simd"]][0] += w["bc"] >= 0
        per[w["simd"]][1] += w["a"] >= 0
        per[w["simd"]][2] += w["d_count"]
    assert per == {0: [4, 2, 0], 1: [3, 2, 5], 2: [3, 2, 5], 3: [3, 2, 6]}
