// render_kernels.hip — mz_render: render.render_top_down (mujoco_maze_amd/render.py) for a batch of env states, on the device.
//
// One workgroup of 256 threads per (image, 64 x 32 pixel tile).  The first wavefront builds the env's primitive list
// (mz_render.h: lane k builds primitive k), keeps those whose conservative pixel box meets the tile and compacts them into LDS
// in drawing order; the other waves meanwhile put the tile's 64 column and 32 row coordinates, and the nearest maze cell of
// each, into LDS (float64 divisions per column and row instead of per pixel).  Then each thread classifies 4 consecutive pixels of a row per pass — primitives in reverse
// order, first hit wins, most of them rejected by their box (mz_render.h), then the 3 x 3 cells around the pixel — and writes their 12 bytes as three 32-bit stores where the
// address allows, byte stores otherwise.
//
// Float64 throughout and built without the relaxed flags of the step kernels (csrc/Makefile: $(BASE) -ffp-contract=off): a
// reciprocal division or a contracted multiply-add changes which pixels lie on an edge.
#include <hip/hip_runtime.h>

#include "mz_internal.h"
#include "mz_render.h"

namespace {

constexpr int kTileW = 64, kTileH = 32, kThreads = 256;  // 64 x 32 beat 64 x 64 and 64 x 16 on both image sizes of tools/render_bench.py
constexpr int kRowsPerPass = kThreads / (kTileW / 4);  // 16

__global__ __launch_bounds__(kThreads) void render_top_down_kernel(RenderDev R, RenderCanvas c, int n_env, int tiles_x, int tiles,
                                                                   const float* __restrict__ qpos, int qpos_by_env,
                                                                   const int* __restrict__ env_idx, const double* __restrict__ env_goals,
                                                                   uint8_t* __restrict__ rgb) {
  __shared__ RenderPrim P[MZR_MAX_PRIM];
  __shared__ double Xs[kTileW], Ys[kTileH];
  __shared__ int Jc[kTileW], Ic[kTileH];
  __shared__ int s_np;
  const int img = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)img * (unsigned)tiles);
  const int tx0 = (tile % tiles_x) * kTileW, ty0 = (tile / tiles_x) * kTileH;
  const int env = env_idx ? env_idx[img] : img;
  const bool ok = env >= 0 && env < n_env;  // an index outside the batch draws an all-zero image and reads nothing
  const int t = (int)threadIdx.x;
  if (t < 64) {
    RenderPrim p;
    bool keep = false;
    if (ok && t < mzr_nprim(R)) {
      const float* q = qpos + (size_t)(qpos_by_env ? env : img) * R.nq;
      const double* goals = env_goals ? env_goals + (size_t)env * MZ_MAX_GOAL * 3 : nullptr;
      mzr_prim(R, c, q, goals, t, &p);
      keep = mzr_meets(p, c, tx0, tx0 + kTileW - 1, ty0, ty0 + kTileH - 1);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) P[__popcll(m & ((1ull << t) - 1ull))] = p;
    if (t == 0) s_np = ok ? (int)__popcll(m) : -1;
  } else if (t < 64 + kTileW) {
    const double X = mzr_px(c, tx0 + t - 64);
    Xs[t - 64] = X;
    Jc[t - 64] = mzr_cell_near(X, R.tx, R.scale, R.cols);
  } else if (t < 64 + kTileW + kTileH) {
    const double Y = mzr_py(c, ty0 + t - 64 - kTileW);
    Ys[t - 64 - kTileW] = Y;
    Ic[t - 64 - kTileW] = mzr_cell_near(Y, R.ty, R.scale, R.rows);
  }
  __syncthreads();
  const int np = s_np;
  const int cx = (t & (kTileW / 4 - 1)) * 4, x = tx0 + cx;
  if (x >= c.w) return;
  const int nx = c.w - x < 4 ? c.w - x : 4;
  for (int ry = t / (kTileW / 4); ry < kTileH; ry += kRowsPerPass) {
    const int y = ty0 + ry;
    if (y >= c.h) break;
    uint32_t col[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (np >= 0 && i < nx) col[i] = mzr_pixel(R, P, np, Xs[cx + i], Ys[ry], Ic[ry], Jc[cx + i]);
    uint8_t* o = rgb + (((size_t)img * c.h + y) * c.w + x) * 3;
    if (nx == 4 && ((uintptr_t)o & 3u) == 0) {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
      o4[0] = col[0] | col[1] << 24;
      o4[1] = col[1] >> 8 | col[2] << 16;
      o4[2] = col[2] >> 16 | col[3] << 8;
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (i < nx) {
          o[3 * i] = (uint8_t)(col[i] & 255u);
          o[3 * i + 1] = (uint8_t)(col[i] >> 8 & 255u);
          o[3 * i + 2] = (uint8_t)(col[i] >> 16 & 255u);
        }
    }
  }
}

}  // namespace

hipError_t mzk_render(mz_handle* h, hipStream_t st, const RenderDev* R, const float* qpos, int qpos_by_env, const int* env_idx, int count,
                      int width, int height, uint8_t* rgb) {
  const RenderCanvas c = mzr_canvas(*R, width, height);
  const int tiles_x = (width + kTileW - 1) / kTileW, tiles_y = (height + kTileH - 1) / kTileH;
  const int tiles = tiles_x * tiles_y;
  const size_t blocks = (size_t)count * (size_t)tiles;
  if (blocks == 0) return hipSuccess;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(render_top_down_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, *R, c, h->n, tiles_x, tiles, qpos, qpos_by_env,
                     env_idx, h->env_goals, rgb);
  return hipGetLastError();
}
