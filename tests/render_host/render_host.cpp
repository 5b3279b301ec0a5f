// Host build of mz_render.h (TEST INFRASTRUCTURE ONLY): the drawing code of the device renderer (render_kernels.hip, mz_render)
// evaluated image by image on the CPU, so that tests/test_render_host.py can compare it with render.render_top_down on a
// machine without a GPU.
#include <stdio.h>

#include "../../mujoco_maze_amd/csrc/mz_render.h"

// one whole image, uint8 [h][w][3], pixel by pixel as the kernel classifies them
static void render_image(const RenderDev& R, const float* q, const double* goals, int w, int h, uint8_t* out) {
  const RenderCanvas c = mzr_canvas(R, w, h);
  RenderPrim P[MZR_MAX_PRIM];
  const int np = mzr_nprim(R);
  for (int k = 0; k < np; k++) mzr_prim(R, c, q, goals, k, &P[k]);
  for (int ys = 0; ys < h; ys++) {
    const double Y = mzr_py(c, ys);
    const int ic = mzr_cell_near(Y, R.ty, R.scale, R.rows);
    for (int xs = 0; xs < w; xs++) {
      const double X = mzr_px(c, xs);
      const uint32_t rgb = mzr_pixel(R, P, np, X, Y, ic, mzr_cell_near(X, R.tx, R.scale, R.cols));
      uint8_t* o = out + ((size_t)ys * w + xs) * 3;
      o[0] = (uint8_t)(rgb & 255u);
      o[1] = (uint8_t)(rgb >> 8 & 255u);
      o[2] = (uint8_t)(rgb >> 16 & 255u);
    }
  }
}

extern "C" {

// n images of width x height into out (uint8 [n][height][width][3]) from the qpos rows [n][nq] (float32); env_goals: per-env goal
// rows [n][MZ_MAX_GOAL][3] (float64) or NULL for the model's goal table.  MZ_OK or an MZ_ERR_* code with a message in err.
int mzr_host_render(const mz_model* m, const float* qpos, const double* env_goals, int n, int ngoal_style, const uint8_t* goal_rgb,
                    const double* goal_size, int width, int height, uint8_t* out, char* err, int errlen) {
  if (ngoal_style != m->ngoal || width < 2 || height < 2 || n < 0) {
    snprintf(err, (size_t)errlen, "bad arguments");
    return MZ_ERR_ARG;
  }
  RenderDev R;
  const char* why = nullptr;
  const int rc = render_dev_from_model(m, goal_rgb, goal_size, &R, &why);
  if (rc != MZ_OK) {
    snprintf(err, (size_t)errlen, "%s", why ? why : "unsupported model");
    return rc;
  }
  for (int i = 0; i < n; i++)
    render_image(R, qpos + (size_t)i * m->nq, env_goals ? env_goals + (size_t)i * MZ_MAX_GOAL * 3 : nullptr, width, height,
                 out + (size_t)i * height * width * 3);
  return MZ_OK;
}

}  // extern "C"
