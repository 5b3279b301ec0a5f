// diverged_main.cpp — diverged states through the kernel source under host sanitizers (TEST INFRASTRUCTURE).
//
// A stand-alone program around the emulation entry points of ant_emu.cpp (the same kernel headers, one lane): built by
// `make diverged_main` with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all, so that any report
// ends the program with a non-zero status.  tests/test_diverged_states.py writes compiled models to files and runs it.
//
//   diverged_main MODEL.bin [MODEL.bin ...]   per model: 200 healthy random-action steps (the control), then from qpos0 one
//                                             state entry at a time overwritten with each poison value, 3 steps each
//   diverged_main --cells V [V ...]           mz_cell of each V: one line "V <double overload> <float overload>"
//
// What a diverged state must satisfy: the step returns (every loop of the kernel source ends whatever the state holds), no
// sanitizer report, and an env whose returned state holds a non-finite entry or |x| >= 1e10 has MZ_STATUS_BAD_STATE set —
// wherever the emulation entry computes that bit (the Point's is set in planar_kernels.hip, not in the code compiled here).
#include <float.h>
#include <stdio.h>
#include <time.h>

#include <string>
#include <vector>

#include "ant_emu.cpp"

namespace {

enum Engine { E_ANT, E_POINT, E_SWIMMER, E_GENERIC };
const char* const ENGINE_NAME[] = {"ant", "point", "swimmer", "general"};

struct Env {
  const mz_model* m;
  Engine eng;
  // exact-size heap arrays: an access past an env's row is an AddressSanitizer report
  std::vector<float> qpos, qvel, warm, act, obs;
  float reward, info[4];
  uint8_t done;
  int32_t t, goal, status, iters;

  explicit Env(const mz_model* model) : m(model) {
    eng = (m->engine == 1 || m->robot == MZ_ROBOT_GENERIC) ? E_GENERIC
          : m->robot == MZ_ROBOT_ANT ? E_ANT : m->robot == MZ_ROBOT_POINT ? E_POINT : E_SWIMMER;
    qpos.resize(m->nq); qvel.resize(m->nv); warm.resize(m->nv); act.resize(m->nu); obs.resize(m->obs_dim);
    reset();
  }
  void reset() {
    for (int i = 0; i < m->nq; i++) qpos[i] = (float)m->qpos0[i];
    for (int i = 0; i < m->nv; i++) qvel[i] = warm[i] = 0.f;
    t = 0; status = 0; goal = -1; done = 0; reward = 0.f;
  }
  int step() {
    switch (eng) {
      case E_ANT: return emu_ant_env_step(m, 1, qpos.data(), qvel.data(), warm.data(), &t, act.data(), obs.data(), &reward, &done, &goal, info, &status, &iters, 0, 0.f, -1.f);
      case E_POINT: return emu_point_env_step(m, 1, qpos.data(), qvel.data(), &t, act.data(), obs.data(), &reward, &done, &goal, &status);
      case E_SWIMMER: return emu_swimmer_env_step(m, 1, qpos.data(), qvel.data(), &t, act.data(), obs.data(), &reward, &done, &goal, info, &status);
      default: {
        char err[256] = "";
        const int rc = emu_generic_env_step(m, 1, qpos.data(), qvel.data(), warm.data(), &t, act.data(), obs.data(), &reward, &done, &goal, info, &status, err, sizeof(err));
        if (rc != MZ_OK) fprintf(stderr, "general engine: %s\n", err);
        return rc;
      }
    }
  }
  bool diverged() const {
    for (float x : qpos) if (!(fabsf(x) < 1e10f)) return true;
    for (float x : qvel) if (!(fabsf(x) < 1e10f)) return true;
    return false;
  }
};

struct Entry { std::string name; bool vel; int idx; };

bool movable_body(const mz_model* m, int body) {
  for (int k = 0; k < m->nblock; k++) if (m->block_bodyid[k] == body) return true;
  for (int k = 0; k < m->nball; k++) if (m->ball_bodyid[k] == body) return true;
  return false;
}

// x, y, z and one quaternion component where the root is a free joint, the robot's first hinge (the Point's heading), the first
// slide of a movable block or ball (or the x of a ball on a free joint) — and one velocity of each of the same classes
std::vector<Entry> entries(const mz_model* m) {
  std::vector<Entry> pos;
  pos.push_back({"x", false, 0});
  pos.push_back({"y", false, 1});
  const bool free_root = m->njnt > 0 && m->jnt_type[0] == MZ_JNT_FREE;
  if (free_root) { pos.push_back({"z", false, 2}); pos.push_back({"quat", false, 4}); }
  int hinge = -1, slide = -1, ball = -1;
  for (int j = 0; j < m->njnt; j++) {
    const bool mov = movable_body(m, m->jnt_bodyid[j]);
    if (hinge < 0 && !mov && m->jnt_type[j] == MZ_JNT_HINGE) hinge = j;
    if (slide < 0 && mov && m->jnt_type[j] == MZ_JNT_SLIDE) slide = j;
    if (ball < 0 && mov && m->jnt_type[j] == MZ_JNT_FREE) ball = j;  // the Ant's billiard ball rolls on a free joint: its x
  }
  if (hinge >= 0) pos.push_back({"hinge", false, m->jnt_qposadr[hinge]});
  if (slide >= 0) pos.push_back({"slide", false, m->jnt_qposadr[slide]});
  else if (ball >= 0) pos.push_back({"ball", false, m->jnt_qposadr[ball]});
  std::vector<Entry> all = pos;
  for (const Entry& e : pos) {
    int d = e.idx;  // slides of the root: qpos index = dof index
    if (e.name == "quat") d = 4;  // an angular velocity of the free root
    else if (e.name == "hinge") d = m->jnt_dofadr[hinge];
    else if (e.name == "slide") d = m->jnt_dofadr[slide];
    else if (e.name == "ball") d = m->jnt_dofadr[ball];
    all.push_back({"v" + e.name, true, d});
  }
  return all;
}

struct Lcg {
  uint64_t s;
  double uniform() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
};

void set_actions(Env& e, Lcg* rng) {
  const mz_model* m = e.m;
  for (int u = 0; u < m->nu; u++) {
    const double lo = m->act_ctrllimited[u] ? m->act_ctrlrange[u][0] : -1.0, hi = m->act_ctrllimited[u] ? m->act_ctrlrange[u][1] : 1.0;
    e.act[u] = (float)(rng ? lo + (hi - lo) * rng->uniform() : 0.25 * hi);
  }
}

double now() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

int run_model(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "%s: cannot open\n", path); return 2; }
  std::vector<unsigned char> raw(sizeof(mz_model) + 1);
  const size_t got = fread(raw.data(), 1, raw.size(), f);
  fclose(f);
  if (got != sizeof(mz_model)) { fprintf(stderr, "%s: %zu bytes, mz_model has %zu\n", path, got, sizeof(mz_model)); return 2; }
  mz_model* m = (mz_model*)malloc(sizeof(mz_model));
  memcpy(m, raw.data(), sizeof(mz_model));
  if (m->abi_version != MZ_ABI_VERSION) { fprintf(stderr, "%s: abi_version %d, built for %d\n", path, m->abi_version, MZ_ABI_VERSION); free(m); return 2; }
  int fail = 0;
  {
    Env e(m);
    const double t0 = now();
    // ---- control: healthy random-action steps stay healthy
    Lcg rng{12345};
    for (int k = 0; k < 200 && !fail; k++) {
      set_actions(e, &rng);
      const int rc = e.step();
      if (rc != MZ_OK) { fprintf(stderr, "%s: control step %d returned %d\n", path, k, rc); fail = 2; }
      else if (e.diverged() || (e.eng != E_POINT && (e.status & MZ_STATUS_BAD_STATE))) {
        fprintf(stderr, "%s: control step %d left a bad state (status %d)\n", path, k, e.status); fail = 3;
      }
    }
    const double t1 = now();
    // ---- one entry at a time, each poison value, 3 steps (what blows up inside a step is met as Inf before it is NaN)
    const float poison[] = {NAN, INFINITY, -INFINITY, 1e12f, -1e12f, 1e30f, -1e30f, FLT_MAX, -FLT_MAX};
    const std::vector<Entry> ent = entries(m);
    int ncase = 0, nflag = 0;
    for (const Entry& en : ent)
      for (float p : poison) {
        if (fail) break;
        e.reset();
        (en.vel ? e.qvel : e.qpos)[en.idx] = p;
        set_actions(e, nullptr);
        ncase++;
        for (int k = 0; k < 3 && !fail; k++) {
          const int rc = e.step();
          if (rc != MZ_OK) { fprintf(stderr, "%s: %s[%d] = %g, step %d returned %d\n", path, en.name.c_str(), en.idx, (double)p, k, rc); fail = 2; break; }
          const bool div = e.diverged();
          nflag += div;
          if (div && e.eng != E_POINT && !(e.status & MZ_STATUS_BAD_STATE)) {
            fprintf(stderr, "%s: %s[%d] = %g, step %d: diverged state without MZ_STATUS_BAD_STATE (status %d)\n", path, en.name.c_str(), en.idx, (double)p, k, e.status);
            fail = 3;
          }
        }
      }
    std::string names;
    for (const Entry& en : ent) names += (names.empty() ? "" : " ") + en.name;
    printf("%s: engine %s, control 200 steps %.2f s, %d cases x 3 steps %.2f s (%d diverged results), entries: %s\n", path, ENGINE_NAME[e.eng], t1 - t0,
           ncase, now() - t1, nflag, names.c_str());
  }
  free(m);
  return fail;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "--cells") {
    for (int i = 2; i < argc; i++) {
      const double v = strtod(argv[i], nullptr);
      const float vf = fabs(v) > (double)FLT_MAX ? (float)copysign((double)INFINITY, v) : (float)v;
      printf("%s %d %d\n", argv[i], mz_cell(v), mz_cell(vf));
    }
    return 0;
  }
  if (argc < 2) { fprintf(stderr, "usage: %s MODEL.bin [...] | --cells V [...]\n", argv[0]); return 2; }
  const double t0 = now();
  for (int i = 1; i < argc; i++) {
    const int rc = run_model(argv[i]);
    if (rc) return rc;
  }
  printf("total %.2f s\n", now() - t0);
  return 0;
}
