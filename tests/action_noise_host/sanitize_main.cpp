// sanitize_main.cpp — the two noise modes of mz_policy.h under the host sanitizers (TEST INFRASTRUCTURE; `make sanitize` builds and
// runs it with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all).  A stand-alone program: nothing here is
// loaded into Python.  Every array is an exact-size heap allocation, so a read or write past a row is an AddressSanitizer report;
// log_std runs through NaN, +-inf and a value whose expf overflows, the observations through NaN and +-inf.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "action_noise_host.cpp"

int main() {
  const int shapes[][3] = {{0, 0, 0}, {1, 5, 0}, {1, 64, 0}, {2, 5, 3}, {2, 64, 64}};
  const float specials[] = {NAN, INFINITY, -INFINITY, 100.0f, -100.0f, 2.0f, 0.0f};
  long checked = 0;
  for (const auto& sh : shapes)
    for (int obs_dim : {1, 7, 123})
      for (int nu : {1, 2, 8})
        for (int activation : {MZ_ACT_TANH, MZ_ACT_RELU})
          for (int squash = 0; squash <= 1; squash++)
            for (int mode : {MZ_NOISE_PRE_SQUASH, MZ_NOISE_ACTION}) {
              const int rows = 9;
              const mzp_shape s{sh[0], sh[1], sh[2], activation};
              const int count = mzp_net_param_count(obs_dim, nu, s) + nu;
              std::vector<float> par((size_t)rows * count), obs((size_t)rows * obs_dim), act((size_t)rows * nu), logp(rows);
              std::vector<unsigned long long> slots(rows);
              for (size_t i = 0; i < par.size(); i++) par[i] = 0.01f * (float)((int)(i * 2654435761u % 201u) - 100);
              for (size_t i = 0; i < obs.size(); i++) obs[i] = 0.03f * (float)((int)(i * 40503u % 201u) - 100);
              for (int r = 0; r < rows; r++) {
                slots[r] = r == 8 ? ~0ULL : (unsigned long long)r * 1000003ULL;
                if (r < 7) par[(size_t)r * count + count - 1] = specials[r];  // log_std of the last unit
              }
              obs[0] = NAN;
              if (obs_dim > 1) { obs[obs_dim] = INFINITY; obs[2 * obs_dim + 1] = -INFINITY; }
              const int legacy = sh[0] <= 1 && activation == MZ_ACT_TANH;
              for (int via_legacy = 0; via_legacy <= legacy; via_legacy++) {
                const int rc = mzp_host_noise_sample(via_legacy, par.data(), count, obs_dim, nu, sh[0], sh[1], sh[2], activation, squash, 1.0, mode, 77ULL, ~0ULL,
                                                     slots.data(), obs.data(), rows, act.data(), logp.data());
                if (rc != MZ_OK) { printf("refused: rc %d\n", rc); return 1; }
                if (squash && mode == MZ_NOISE_ACTION)
                  for (float a : act)
                    if (!(isnan(a) || fabsf(a) <= 1.0f)) { printf("an action outside the range: %g\n", a); return 1; }
                checked += rows;
              }
            }
  printf("action_noise_host under the sanitizers: %ld rows, no report\n", checked);
  return 0;
}
