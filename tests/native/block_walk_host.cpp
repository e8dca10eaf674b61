// TEST INFRASTRUCTURE ONLY: host build of the tile walks of conv_block32s_kernel (classifier-pipeline_amd/csrc/
// cpx_conv_layout_core.h: walk_tile, choose_walk; tests/test_block_walk_host.py).  It walks a launch the way the kernel's
// workgroups do -- tile j = 0, 1, .. of every workgroup until the first one that does not exist -- and counts what the
// kernel's carry condition would see.  With -DBLOCK_WALK_HOST_MAIN it is a program of its own, for a sanitizer build.
// The product never loads either.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "cpx_conv_layout_core.h"

// grid: what CPX_BLOCK32_GRID (or CUs / groups) asks for; walk: cpx::WALK_TILES, cpx::WALK_ROWS, or -1 = the launcher's choice.
// out: the walk taken, grid width, total tiles, tiles visited at least once, visits beyond the first, tiles outside [0, total),
// carried tiles (same sample and tile row as the workgroup's previous tile, one column to its left), the largest and the
// smallest per-workgroup tile count.  Returns fill_tiles' code.
extern "C" int block_walk_host(int tiles_x, int tiles_y, long long n, int grid, int walk, int64_t* out) {
  cpx::BlkTiles td{};
  if (const int rc = cpx::fill_tiles(td, tiles_x, tiles_y, n, cpx::TILES_PERSISTENT)) return rc;
  const int gx = cpx::persistent_grid_x(grid, 1, td.total);
  cpx::set_walk(td, walk < 0 ? cpx::choose_walk(td, gx) : walk);
  std::vector<unsigned char> seen((size_t)td.total, 0);
  int64_t visited = 0, again = 0, outside = 0, carried = 0, most = 0, least = td.total;
  for (int bx = 0; bx < gx; ++bx) {
    int pn = -1, pty = -1, ptx = -1, count = 0;
    for (int j = 0;; ++j) {
      int sn, ty, tx;
      if (!cpx::walk_tile(td, bx, gx, j, sn, ty, tx)) break;
      ++count;
      if (sn < 0 || sn >= n || ty < 0 || ty >= tiles_y || tx < 0 || tx >= tiles_x) {
        ++outside;
      } else {
        unsigned char& s = seen[((size_t)sn * tiles_y + ty) * tiles_x + tx];
        s ? ++again : ++visited;
        s = 1;
      }
      if (j > 0 && sn == pn && ty == pty && tx + 1 == ptx) ++carried;  // (the kernel: n0 == n1 && oy0 == oy1 && ox1 + 16 == ox0)
      pn = sn, pty = ty, ptx = tx;
    }
    most = count > most ? count : most;
    least = count < least ? count : least;
  }
  const int64_t v[9] = {td.walk, gx, td.total, visited, again, outside, carried, most, least};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  return 0;
}

extern "C" long long walk_max_tiles_host(int tiles_x, int tiles_y, long long n, int walk, int gx) {
  cpx::BlkTiles td{};
  if (cpx::fill_tiles(td, tiles_x, tiles_y, n, cpx::TILES_PERSISTENT)) return -1;
  return cpx::walk_max_tiles(td, walk, gx);
}
extern "C" double walk_carry_saving_host() { return cpx::WALK_CARRY_SAVING; }

#ifdef BLOCK_WALK_HOST_MAIN
namespace {
int failures = 0;
#define EXPECT(cond)                                     \
  do {                                                   \
    if (!(cond)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      ++failures;                                        \
    }                                                    \
  } while (0)
}  // namespace

int main() {
  const int shapes[][2] = {{1, 1}, {2, 2}, {3, 3}, {10, 10}, {10, 3}, {3, 10}};
  for (const auto& sh : shapes)
    for (long long n : {1ll, 3ll, 7ll, 1559ll})
      for (int grid : {8, 24, 128, 4096})
        for (int walk : {-1, (int)cpx::WALK_TILES, (int)cpx::WALK_ROWS}) {
          int64_t o[9];
          EXPECT(block_walk_host(sh[0], sh[1], n, grid, walk, o) == 0);
          const int64_t total = (int64_t)sh[0] * sh[1] * n;
          EXPECT(o[2] == total && o[3] == total && o[4] == 0 && o[5] == 0);
          EXPECT(walk < 0 || o[0] == walk);
          EXPECT(o[7] == walk_max_tiles_host(sh[0], sh[1], n, (int)o[0], (int)o[1]));
          if (o[0] == cpx::WALK_TILES) EXPECT(o[6] == 0);  // (a workgroup's tiles ascend: never a left neighbour next)
        }
  int64_t o[9];
  EXPECT(block_walk_host(10, 10, 1559, 128, -1, o) == 0 && o[0] == cpx::WALK_ROWS && o[6] == 1559 * 90 && o[7] == 1220);
  EXPECT(block_walk_host(10, 10, 3, 128, -1, o) == 0 && o[0] == cpx::WALK_TILES);
  EXPECT(block_walk_host(4096, 1, 1, 8, -1, o) == -3);
  return failures ? 1 : 0;
}
#endif
