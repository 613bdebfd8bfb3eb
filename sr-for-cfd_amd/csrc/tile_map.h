// Where one output row (or column) of an overlapped tiling comes from.  The ONE statement of the per-axis source map: tile_plan.cpp
// and tools/tile_plan_check.cpp compile it for the host, tiles.hip runs it in the blending stitch.
//
// Along an axis, T tiles of `fine` output rows each start every `stride` rows and share `overlap = fine - stride` rows with the next
// one (0 <= 2 * overlap <= fine, so a row lies in at most two tiles); the axis has T * stride + overlap rows.  Row R:
//   t1 = min(R / stride, T - 1), r1 = R - t1 * stride
//   t1 >= 1 and r1 < overlap: blended from tile t1 - 1 at row r1 + stride (value a) and tile t1 at row r1 (value b) with the ramp
//                             weight w[r1]: a + w * (b - a)
//   otherwise:                tile t1, row r1, copied.
#pragma once

#if defined(__HIP__)
#define SRCFD_TILE_HD __host__ __device__
#else
#define SRCFD_TILE_HD
#endif

namespace srcfd {

struct TileAxisSrc {
  int t0, r0;   // the earlier tile and its row (value a); t0 < 0: the row has one source and nothing is computed along this axis
  int t1, r1;   // the tile the row belongs to and its row there (value b, or the value copied)
  int j;        // index into the ramp table when blended, else -1
};

SRCFD_TILE_HD inline TileAxisSrc tile_axis_src(int R, int T, int stride, int overlap) {
  int t1 = R / stride;
  if (t1 > T - 1) t1 = T - 1;
  const int r1 = R - t1 * stride;
  if (t1 >= 1 && r1 < overlap) return TileAxisSrc{t1 - 1, r1 + stride, t1, r1, r1};
  return TileAxisSrc{-1, 0, t1, r1, -1};
}

}  // namespace srcfd
