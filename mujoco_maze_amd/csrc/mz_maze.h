// mz_maze.h — the maze's cell grid as the kernels see it (MazeDev: one bitmask per row), its derivation from the compiled
// `mz_model` (include/mazestep.h), the row lookup, and the contact of two grid-aligned boxes (wall / platform cells and
// movable blocks never rotate).
//
// Plain C++ (no HIP): shared by the kernel translation units and the CPU emulation in tests/emu/.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mazestep.h"
#include "mz_lanes.h"

struct MazeDev {
  int rows, cols;
  uint32_t rowmask[MZ_MAX_GRID];  // bit j set <=> cell (i, j) is a BLOCK
  float scale, tx, ty, half_xy, half_z, center_z;
  // elevated mazes (Fall / MultiFall): a platform box (same footprint, z from 0 to 2 half_z, centre half_z) under every cell
  // of the grid that is not a CHASM; the walls stand on top (center_z = half_z + height offset)
  int elevated;
  uint32_t platmask[MZ_MAX_GRID];  // bit j set <=> cell (i, j) carries a platform
};

static inline void maze_dev_from_model(MazeDev* z, const mz_model* m) {
  memset(z, 0, sizeof(*z));
  z->rows = m->grid_rows; z->cols = m->grid_cols;
  for (int i = 0; i < m->grid_rows; i++)
    for (int j = 0; j < m->grid_cols; j++)
      if (m->grid[i][j] == MZ_CELL_BLOCK) z->rowmask[i] |= (1u << j);
  z->elevated = m->elevated;
  for (int i = 0; i < m->grid_rows && m->elevated; i++)
    for (int j = 0; j < m->grid_cols; j++)
      if (m->grid[i][j] != MZ_CELL_CHASM) z->platmask[i] |= (1u << j);
  z->scale = (float)m->maze_scale; z->tx = (float)m->torso_x; z->ty = (float)m->torso_y;
  z->half_xy = (float)m->wall_half_xy; z->half_z = (float)m->wall_half_z; z->center_z = (float)m->wall_center_z;
}

// Cell index of a floating cell coordinate (world coordinate / scale + 0.5, from an env's STATE): floor, clamped in floating
// point to [-2, MZ_MAX_GRID + 1] before the conversion, NaN -> -2.  A diverged state (NaN, Inf, 1e30) must not reach the
// float -> int conversion: in C++ a value outside int's range is undefined, x86 returns INT_MIN, the device's conversion
// saturates (Inf -> INT_MAX, NaN -> 0) — and a cell loop `for (i = i0; i <= i1; i++)` with i1 == INT_MAX never ends.  With
// this every cell range is at most MZ_MAX_GRID + 4 long on any platform.  Cells outside the grid are skipped by every caller
// (two cells of room on each side: the 3 x 3 neighbourhoods of a cell just outside the grid still reach into it), so for a
// state in range nothing changes by a bit.
MZ_HD int mz_cell(double f) {
  f = floor(f);
  if (!(f >= -2.0)) return -2;
  return f > (double)(MZ_MAX_GRID + 1) ? MZ_MAX_GRID + 1 : (int)f;
}
MZ_HD int mz_cell(float f) {
  f = floorf(f);
  if (!(f >= -2.0f)) return -2;
  return f > (float)(MZ_MAX_GRID + 1) ? MZ_MAX_GRID + 1 : (int)f;
}

// Row bitmask of the cell grid for a per-lane row index.  The grid lives in the kernel-argument block
// (scalar registers); a select chain keeps it there — indexing the array with a vector index would make the
// compiler spill it to scratch memory.
MZ_HD uint32_t maze_row(const MazeDev& z, int i) {
  uint32_t m = 0u;
#pragma unroll
  for (int r = 0; r < MZ_MAX_GRID; r++) m = (r == i) ? z.rowmask[r] : m;
  return m;
}

// Two axis-aligned boxes (movable blocks never rotate, maze cells are grid-aligned): MuJoCo's mjc_BoxBox as restated in
// oracle/mzo_physics.c box_box, specialised to parallel axes, in float64 on WORLD coordinates (grid-aligned boxes sit on exact
// ties — a block at its spawn position shares border lines with the diagonal wall cells, its z extent equals the walls' —
// which fp32 torso-relative coordinates would decide at random).  Separating axis = the face axis of least penetration
// (first of x, y, z on ties; an edge-edge axis never wins between parallel boxes), dist = -penetration; contact points = the
// corners of the intersection of the two facing faces (inclusive border tests); an intersection without area — boxes that share
// only a border line: a block at its spawn position and the diagonal wall cells — makes no contact [ASSUME-12].
// Box 1 = geom1: the normal points from box 1 to box 2.
#define MZ_BOX_MINOVERLAP 1e-6
struct AlignedBB { int ax, nu, nv; double dist, sg, pa, pu[2], pv[2]; };  // (pu / pv: read through selects, never by a run-time index — an indexed read put the struct into scratch memory)
MZ_HD bool aligned_box_box(const double* c1, const double* h1, const double* c2, const double* h2, double margin, AlignedBB& o) {
  double pen[3];
  for (int k = 0; k < 3; k++) { pen[k] = h1[k] + h2[k] - fabs(c2[k] - c1[k]); if (pen[k] < -margin) return false; }
  int ax = 0;
  if (pen[1] < pen[ax]) ax = 1;
  if (pen[2] < pen[ax]) ax = 2;
  const int u = ax == 2 ? 0 : ax + 1, v = ax == 0 ? 2 : ax - 1;
  double lo[3], hi[3];
  for (int k = 0; k < 3; k++) { lo[k] = fmax(c1[k] - h1[k], c2[k] - h2[k]); hi[k] = fmin(c1[k] + h1[k], c2[k] + h2[k]); }
  const double h1u = u == 0 ? h1[0] : (u == 1 ? h1[1] : h1[2]), h1v = v == 0 ? h1[0] : (v == 1 ? h1[1] : h1[2]);
  const double dtol = 1e-9 * (1.0 + h1u + h1v);  // coincident candidates (oracle: same)
  const double lou = u == 0 ? lo[0] : (u == 1 ? lo[1] : lo[2]), hiu = u == 0 ? hi[0] : (u == 1 ? hi[1] : hi[2]);
  const double lov = v == 0 ? lo[0] : (v == 1 ? lo[1] : lo[2]), hiv = v == 0 ? hi[0] : (v == 1 ? hi[1] : hi[2]);
  if (hiu - lou <= MZ_BOX_MINOVERLAP || hiv - lov <= MZ_BOX_MINOVERLAP) return false;  // the faces must overlap by a positive area (oracle: MZO_BOX_MINOVERLAP)
  const double c1a = ax == 0 ? c1[0] : (ax == 1 ? c1[1] : c1[2]), c2a = ax == 0 ? c2[0] : (ax == 1 ? c2[1] : c2[2]);
  const double h1a = ax == 0 ? h1[0] : (ax == 1 ? h1[1] : h1[2]), pa = ax == 0 ? pen[0] : (ax == 1 ? pen[1] : pen[2]);
  o.ax = ax; o.sg = c2a >= c1a ? 1.0 : -1.0; o.dist = -pa;
  o.pa = c1a + o.sg * (h1a + 0.5 * o.dist);
  o.nu = hiu - lou > dtol ? 2 : 1; o.nv = hiv - lov > dtol ? 2 : 1;
  o.pu[0] = lou; o.pu[1] = hiu; o.pv[0] = lov; o.pv[1] = hiv;
  return true;
}
