/* examples/c_abi_fun.c -- a user-defined log-posterior through the C-ABI from plain C: fmcmc_mcmc_run_fun_host() with a
 * batched callback (fmcmc_logpost_fn) that runs on the CPU.  Host pointers only, no Python, no torch.
 *
 *   gcc -O2 -std=gnu11 -ffp-contract=off -mfma -Iinclude examples/c_abi_fun.c -o c_abi_fun -Lfmcmc_amd/lib -lfmcmc_amd -lm \
 *       -Wl,-rpath,$PWD/fmcmc_amd/lib
 *   ./c_abi_fun in.bin out.bin
 *
 * in.bin : int64 n, p, C, k, nsteps, burnin, thin, seed, kind, calls; double X[p][n], y[n], initial[C][k], scale[k], lb[k], ub[k]
 * out.bin: per call: double samples[C][k][S], logpost[C][S], draws[C][k][S]; int64 accept_count[C]; uint32 accept_bits[C][W];
 *          then the carried state: double theta0[C][k], f0[C]; int64 abs_iter[C]; double Sigma[C][k][k], mean_prev[C][k];
 *          int32 have_mean[C], nerrors[C]                    (S = fmcmc_kept_rows(...), W = ceil(nsteps / 32), no fixed parameter)
 * The log-posterior: the Gaussian linear regression of README.md:128-139 (intercept, guard), written in the engine's canonical
 * order -- residual sums of squares over 512 lanes (observation i on lane i mod 512, fma accumulation) combined by a pairwise
 * tree, include/fmh_detmath.h for log -- so that the chains are those of the library's own family.  Any other model goes here
 * the same way.  kind: FMCMC_KERNEL_* (normal, normal_reflective, adapt, ram, unif, unif_reflective); `calls` consecutive calls
 * carry the kernel state from one to the next (fresh = 0), as the bulks of MCMC_with_conv_checker do.
 * Exit code: 0 ok, 2 usage / IO, 3 the library returned an error (message on stderr; no GPU -> FMCMC_ERR_DEVICE).
 */
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fmcmc_amd.h"
#include "fmh_detmath.h"

typedef struct { int64_t n, p; const double* X; const double* y; } linreg;

/* out[c] = sum_i dnorm(y_i - (b0 + x_i b), sd = sigma, log = TRUE) for theta[c] = (b0, b[p], sigma) */
static int linreg_logpost(const double* theta, int64_t nchains, int32_t k, double* out, void* hip_stream, void* user) {
  (void)hip_stream;
  const linreg* m = (const linreg*)user;
  for (int64_t c = 0; c < nchains; c++) {
    const double* th = theta + c * k;
    double acc[512];
    for (int l = 0; l < 512; l++) acc[l] = 0.0;
    for (int64_t i = 0; i < m->n; i++) {
      double mu = th[0];
      for (int64_t j = 0; j < m->p; j++) mu = fmh_fma(m->X[j * m->n + i], th[1 + j], mu);
      const double r = m->y[i] - mu;
      acc[i & 511] = fmh_fma(r, r, acc[i & 511]);
    }
    for (int s = 1; s < 512; s <<= 1)
      for (int l = 0; l < 512; l += 2 * s) acc[l] = acc[l] + acc[l + s];
    const double sigma = th[1 + m->p];
    double f;
    if (sigma < 0.0 || fmh_isnan(sigma)) f = fmh_nan();
    else if (sigma == 0.0) f = -fmh_inf();
    else f = -((double)m->n * (fmh_log(sigma) + FMH_LN_SQRT_2PI)) - (0.5 * acc[0]) / (sigma * sigma);
    out[c] = fmh_isfinite(f) ? f : -fmh_inf();
  }
  return 0;
}

static int rd(void* p, size_t sz, size_t cnt, FILE* f) { return fread(p, sz, cnt, f) == cnt; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  if (fmcmc_abi_version() != FMCMC_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 3; }
  FILE* f = fopen(argv[1], "rb");
  int64_t h[10];
  if (!f || !rd(h, sizeof(int64_t), 10, f)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int64_t n = h[0], p = h[1], C = h[2], k = h[3], nsteps = h[4], burnin = h[5], thin = h[6], calls = h[9];
  if (calls < 1 || k != p + 2) { fprintf(stderr, "need calls >= 1 and k = p + 2\n"); return 2; }
  double* X = malloc(sizeof(double) * (size_t)(p * n)); double* y = malloc(sizeof(double) * (size_t)n);
  double* theta0 = malloc(sizeof(double) * (size_t)(C * k)); double* scale = malloc(sizeof(double) * (size_t)k);
  double* lb = malloc(sizeof(double) * (size_t)k); double* ub = malloc(sizeof(double) * (size_t)k);
  if (!rd(X, sizeof(double), (size_t)(p * n), f) || !rd(y, sizeof(double), (size_t)n, f) ||
      !rd(theta0, sizeof(double), (size_t)(C * k), f) || !rd(scale, sizeof(double), (size_t)k, f) ||
      !rd(lb, sizeof(double), (size_t)k, f) || !rd(ub, sizeof(double), (size_t)k, f)) {
    fprintf(stderr, "short input\n"); return 2;
  }
  fclose(f);
  linreg model = {n, p, X, y};

  double* mu = calloc((size_t)k, sizeof(double)); uint8_t* fixed = calloc((size_t)k, 1);
  fmcmc_kernel kn; memset(&kn, 0, sizeof kn);
  kn.kind = (int32_t)h[8]; kn.k = (int32_t)k; kn.mu = mu; kn.scale = scale; kn.lb = lb; kn.ub = ub; kn.fixed = fixed;
  kn.scheme = FMCMC_SCHEME_JOINT; kn.freq = 1; kn.warmup = (kn.kind == FMCMC_KERNEL_ADAPT) ? 20 : 0; kn.until = 1.0 / 0.0;
  kn.eps = 1e-4; kn.arate = 0.234; kn.nadapt = 4;

  fmcmc_run r; memset(&r, 0, sizeof r);
  r.nchains = C; r.nsteps = nsteps; r.burnin = burnin; r.thin = thin; r.seed = (uint64_t)h[7]; r.rng_mode = FMCMC_RNG_PHILOX;
  if (fmcmc_validate_fun(&kn, &r) != FMCMC_OK) { fprintf(stderr, "fmcmc_validate_fun: %s\n", fmcmc_last_error()); return 3; }
  const int64_t S = fmcmc_kept_rows(nsteps, burnin, thin), W = (nsteps + 31) / 32;

  fmcmc_state st; memset(&st, 0, sizeof st);   /* (kf = k: no fixed parameter) */
  st.theta0 = theta0; st.f0 = calloc((size_t)C, sizeof(double)); st.abs_iter = calloc((size_t)C, sizeof(int64_t));
  st.Sigma = calloc((size_t)(C * k * k), sizeof(double)); st.mean_prev = calloc((size_t)(C * k), sizeof(double));
  st.have_mean = calloc((size_t)C, sizeof(int32_t)); st.nerrors = calloc((size_t)C, sizeof(int32_t));
  st.fresh = 1;
  fmcmc_out out; memset(&out, 0, sizeof out);
  out.samples = malloc(sizeof(double) * (size_t)(C * k * S)); out.logpost = malloc(sizeof(double) * (size_t)(C * S));
  out.draws = malloc(sizeof(double) * (size_t)(C * k * S)); out.accept_bits = calloc((size_t)(C * W), sizeof(uint32_t));
  out.accept_count = calloc((size_t)C, sizeof(int64_t)); out.status = calloc((size_t)C, sizeof(int32_t));
  out.status_step = calloc((size_t)C, sizeof(int64_t)); out.status_theta = calloc((size_t)(C * k), sizeof(double));

  FILE* fo = NULL;
  for (int64_t call = 0; call < calls; call++) {
    const int rc = fmcmc_mcmc_run_fun_host(&kn, &r, &st, &out, linreg_logpost, &model, 0 /* device */);
    if (rc != FMCMC_OK) { fprintf(stderr, "fmcmc_mcmc_run_fun_host: rc = %d: %s\n", rc, fmcmc_last_error()); return 3; }
    r.step_base += nsteps;   /* (the next call continues the chains' step counter: a new stretch of the stream) */
    if (!fo && !(fo = fopen(argv[2], "wb"))) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fwrite(out.samples, sizeof(double), (size_t)(C * k * S), fo);
    fwrite(out.logpost, sizeof(double), (size_t)(C * S), fo);
    fwrite(out.draws, sizeof(double), (size_t)(C * k * S), fo);
    fwrite(out.accept_count, sizeof(int64_t), (size_t)C, fo);
    fwrite(out.accept_bits, sizeof(uint32_t), (size_t)(C * W), fo);
    printf("call %lld: kernel %s, chain 0 accepted %lld of %lld\n", (long long)call, fmcmc_last_kernel(),
           (long long)out.accept_count[0], (long long)(nsteps - 1));
  }
  fwrite(st.theta0, sizeof(double), (size_t)(C * k), fo);
  fwrite(st.f0, sizeof(double), (size_t)C, fo);
  fwrite(st.abs_iter, sizeof(int64_t), (size_t)C, fo);
  fwrite(st.Sigma, sizeof(double), (size_t)(C * k * k), fo);
  fwrite(st.mean_prev, sizeof(double), (size_t)(C * k), fo);
  fwrite(st.have_mean, sizeof(int32_t), (size_t)C, fo);
  fwrite(st.nerrors, sizeof(int32_t), (size_t)C, fo);
  fclose(fo);
  return 0;
}
