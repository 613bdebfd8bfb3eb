// Static schedule of `tail16` (kernels_bf16.hip): which wave of the 1024-thread workgroup runs which BC, A and D items of a round,
// as constexpr functions of the wave number that the kernel calls and that the static_asserts below -- and, from the table that
// tools/tail16_schedule_print.cpp prints, tests/test_tail16_schedule.py -- check on the host.  Plain C++: no HIP header is needed.
//
// A round has 13 BC items (32 columns of the strip's 200 x 2 (100-level pixel, ConvT#3 tap row) columns each), 8 A items and 16 D
// items (output row pair rp = item >> 2, 16-tile group j4 = item & 3).  The kernel is bound by vector-instruction issue and wave w
// runs on SIMD w % 4, so the schedule spreads the items' vector instructions over the SIMDs.  Measured (DESIGN.md 9,
// profiles/tail16_bc13): the SIMD that carries four BC items ends the round, so it carries no D item and not the merged BC item:
//   SIMD 0: 4 BC + 2 A        SIMD 1, 2: 3 BC + 2 A + 5 D each        SIMD 3: 3 BC + 2 A + 6 D
//   waves 0-7  (role P): BC item = wave, A item = wave, no D
//   waves 8-12 (role Q): one BC item each -- wave 9 (SIMD 1) the merged item 12, wave 12 item 9, the others item = wave;
//                        waves 9 and 10 also one D item each, wave 11 a pair of D items, waves 8 and 12 none
//   waves 13-15 (role Q): four D items each, as two interleaved pairs
// BC items 0-11 are (pixel tile t = item >> 1, tap row m3 = item & 1): lane l31 holds pixel 32 t + l31.  Pixel tile 6 would hold
// pixels 192-223 of 200: its eight real pixels are ONE item, 12, that carries both tap rows -- lanes 0-7 hold pixel 192 + l31 with
// m3 = 0, lanes 8-15 the same pixels with m3 = 1, lanes 16-31 nothing.
#pragma once

namespace srcfd {
namespace tail16_sched {

constexpr int WAVES = 16, SIMDS = 4, ROLE_P_WAVES = 8;
constexpr int BC_ITEMS = 13, A_ITEMS = 8, D_ITEMS = 16;
constexpr int BC_MERGED = 12;              // the item that carries both tap rows of pixels 192-199
constexpr int PIXELS = 200, TAP_ROWS = 2;  // columns of a strip at the 100-level: 2 rows of 100 pixels x ConvT#3's two tap rows

constexpr int simd_of(int wave) { return wave & 3; }
constexpr int bc_item(int wave) { return wave == 9 ? 12 : wave == 12 ? 9 : wave < BC_ITEMS ? wave : -1; }
constexpr int a_item(int wave) { return wave < ROLE_P_WAVES ? wave : -1; }

// D items of a wave: d_first .. d_first + min(d_count, 2) - 1, and d_second, d_second + 1 when d_count == 4.
//   wave 9: item 2;  wave 10: item 3;  wave 11: 14, 15
//   wave 13: 0, 1 and 4, 5;  wave 14: 8, 9 and 12, 13;  wave 15: 6, 7 and 10, 11
// What the D code needs (asserted below): a pair is two consecutive items of one row pair; a wave's second pair has the j4 of its
// first (one set of lane offsets serves both) and is never in row pair 0 (sample and segment seams go through d_first only).
constexpr int d_count(int wave) { return wave < 9 ? 0 : wave < 11 ? 1 : wave == 11 ? 2 : wave == 12 ? 0 : 4; }
constexpr int d_first(int wave) { return wave == 9 ? 2 : wave == 10 ? 3 : wave == 11 ? 14 : wave == 13 ? 0 : wave == 14 ? 8 : wave == 15 ? 6 : 0; }
constexpr int d_second(int wave) { return d_count(wave) == 4 ? d_first(wave) + 4 : 0; }

// BC column of lane l31 (0..31) of an item: 100-level pixel of the strip (-1: the lane holds nothing and never stores) and tap row
constexpr int bc_pixel(int item, int l31) { return item < 0 ? -1 : item < BC_MERGED ? 32 * (item >> 1) + l31 : l31 < 16 ? 192 + (l31 & 7) : -1; }
constexpr int bc_tap_row(int item, int l31) { return item < BC_MERGED ? item & 1 : (l31 >> 3) & 1; }

// ---- the checks ----
constexpr bool wave_owns_d(int wave, int item) {
  const int c = d_count(wave), f = d_first(wave), s = d_second(wave);
  return (c >= 1 && item == f) || (c >= 2 && item == f + 1) || (c == 4 && (item == s || item == s + 1));
}
constexpr int d_owners(int item) {
  int n = 0;
  for (int w = 0; w < WAVES; ++w) n += wave_owns_d(w, item) ? 1 : 0;
  return n;
}
constexpr int merged_wave() {
  for (int w = 0; w < WAVES; ++w)
    if (bc_item(w) == BC_MERGED) return w;
  return -1;
}
constexpr bool every_bc_column_once() {
  int owners[PIXELS * TAP_ROWS] = {};
  for (int w = 0; w < WAVES; ++w)
    for (int l = 0; l < 32; ++l) {
      const int px = bc_pixel(bc_item(w), l);
      if (px >= PIXELS) return false;
      if (px >= 0) ++owners[TAP_ROWS * px + bc_tap_row(bc_item(w), l)];
    }
  for (int c = 0; c < PIXELS * TAP_ROWS; ++c)
    if (owners[c] != 1) return false;
  return true;
}
constexpr bool no_bc_lane_outside() {   // a lane holds a pixel of the strip or nothing; BC items 0 .. BC_ITEMS - 1 have one wave each
  for (int i = 0; i < BC_ITEMS; ++i) {
    int owners = 0;
    for (int w = 0; w < WAVES; ++w) owners += bc_item(w) == i ? 1 : 0;
    if (owners != 1) return false;
    for (int l = 0; l < 32; ++l)
      if (bc_pixel(i, l) >= PIXELS) return false;
  }
  return true;
}
constexpr bool every_d_item_once() {
  for (int i = 0; i < D_ITEMS; ++i)
    if (d_owners(i) != 1) return false;
  return true;
}
constexpr bool d_pairs_fit_the_d_code() {
  for (int w = 0; w < WAVES; ++w) {
    const int c = d_count(w), f = d_first(w), s = d_second(w);
    if (c != 0 && c != 1 && c != 2 && c != 4) return false;
    if (c >= 1 && (f < 0 || f + (c >= 2 ? 1 : 0) >= D_ITEMS)) return false;
    if (c >= 2 && (f & 1) != 0) return false;                                                       // a pair: items 2k, 2k + 1 of one row pair
    if (c == 4 && ((s & 1) != 0 || (s & 3) != (f & 3) || (s >> 2) == 0 || s + 1 >= D_ITEMS)) return false;
  }
  return true;
}
constexpr bool role_p_owns_no_d() {
  for (int w = 0; w < ROLE_P_WAVES; ++w)
    if (d_count(w) != 0) return false;
  return true;
}
constexpr int simd_bc(int simd) { int n = 0; for (int w = simd; w < WAVES; w += SIMDS) n += bc_item(w) >= 0 ? 1 : 0; return n; }
constexpr int simd_a(int simd) { int n = 0; for (int w = simd; w < WAVES; w += SIMDS) n += a_item(w) >= 0 ? 1 : 0; return n; }
constexpr int simd_d(int simd) { int n = 0; for (int w = simd; w < WAVES; w += SIMDS) n += d_count(w); return n; }

static_assert(every_bc_column_once(), "every (pixel, tap row) column of the 200 x 2 belongs to exactly one lane of one BC item");
static_assert(no_bc_lane_outside(), "BC items 0-12 have one wave each and no lane past pixel 199");
static_assert(every_d_item_once(), "every D item 0-15 belongs to exactly one wave");
static_assert(d_pairs_fit_the_d_code(), "D pairs: consecutive items of a row pair; a second pair shares its first's j4 and is not in row pair 0");
static_assert(role_p_owns_no_d(), "role P (waves 0-7) has no D state");
static_assert(merged_wave() >= ROLE_P_WAVES && simd_of(merged_wave()) != 0, "the merged item's path exists in role Q's round loop only, and SIMD 0 has four BC items already");
static_assert(a_item(ROLE_P_WAVES - 1) == A_ITEMS - 1 && a_item(ROLE_P_WAVES) < 0, "A items 0-7 on role P");
static_assert(simd_bc(0) == 4 && simd_a(0) == 2 && simd_d(0) == 0, "SIMD 0: 4 BC + 2 A (DESIGN.md 4.1)");
static_assert(simd_bc(1) == 3 && simd_a(1) == 2 && simd_d(1) == 5, "SIMD 1: 3 BC + 2 A + 5 D");
static_assert(simd_bc(2) == 3 && simd_a(2) == 2 && simd_d(2) == 5, "SIMD 2: 3 BC + 2 A + 5 D");
static_assert(simd_bc(3) == 3 && simd_a(3) == 2 && simd_d(3) == 6, "SIMD 3: 3 BC + 2 A + 6 D");

}  // namespace tail16_sched
}  // namespace srcfd
