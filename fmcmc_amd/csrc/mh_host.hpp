// mh_host.hpp -- the staging of the host-pointer entry points (fmcmc_mcmc_run_host, fmcmc_mcmc_run_fun_host): one stream, one
// device block per array of the call, and ONE list of the fields of fmcmc_kernel / fmcmc_run / fmcmc_state / fmcmc_out that
// both entry points move in and out.  Included by mh_engine.hip only.
#pragma once

namespace {

// The device side of one host-pointer call: its sizes, copies of the caller's structs whose pointers become device pointers,
// the stream and the device blocks.  The first failure sticks: `rc` keeps its code (the message is in fmcmc_last_error()) and
// every later step is skipped, so a list of steps needs no check in between.  The destructor synchronises the stream (the
// call's stream-ordered scratch is released before its buffers), frees the blocks, then destroys the stream.
struct HostStage {
  const int k, kf;
  const size_t C, S, nsteps, nwords;
  const bool adaptive, mirror, fresh;
  fmcmc_kernel dk;
  fmcmc_run dr;
  fmcmc_state ds;
  fmcmc_out dout;
  hipStream_t stream = nullptr;
  std::vector<void*> blocks;
  int rc = FMCMC_OK;
  HostStage(const fmcmc_kernel* kn, const fmcmc_run* run, const fmcmc_state* st, const fmcmc_out* out)
      : k(kn->k), kf(count_free(kn, kn->fixed)), C((size_t)run->nchains), S((size_t)fmcmc_kept_rows(run->nsteps, run->burnin, run->thin)),
        nsteps((size_t)run->nsteps), nwords((size_t)((run->nsteps + 31) / 32)),
        adaptive(kn->kind == FMCMC_KERNEL_ADAPT || kn->kind == FMCMC_KERNEL_RAM),
        mirror(kn->kind == FMCMC_KERNEL_NMIRROR || kn->kind == FMCMC_KERNEL_UMIRROR), fresh(st->fresh != 0),
        dk(*kn), dr(*run), ds(*st), dout(*out) { dout.ld_rows = 0; }
  HostStage(const HostStage&) = delete;
  ~HostStage() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : blocks) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
  }
  int check(hipError_t e, const char* call) {
    if (e != hipSuccess && rc == FMCMC_OK) { set_err("%s failed: %s", call, hipGetErrorString(e)); rc = FMCMC_ERR_DEVICE; }
    return rc;
  }
  int open(int device) {
    if (check(hipSetDevice(device), "hipSetDevice(device)") != FMCMC_OK) return rc;
    return check(hipStreamCreate(&stream), "hipStreamCreate(&stream)");
  }
  // a device block of `bytes` (one hipMalloc per array; an empty array still gets a block), filled from `src` unless that is
  // nullptr; its address goes into the pointer at `field`
  int up(void* field, const void* src, size_t bytes) {
    if (rc != FMCMC_OK) return rc;
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) { set_err("hipMalloc(%zu) failed", bytes); return rc = FMCMC_ERR_DEVICE; }
    blocks.push_back(p);
    *(void**)field = p;
    return src ? check(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(host to device)") : rc;
  }
  int fill(void* dst, int byte, size_t bytes) {
    return rc != FMCMC_OK ? rc : check(hipMemsetAsync(dst, byte, bytes, stream), "hipMemsetAsync");
  }
  int down(void* dst, const void* src, size_t bytes) {
    return rc != FMCMC_OK ? rc : check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(device to host)");
  }
  // one array of a list that serves both directions: back = false allocates its block at `field` (and uploads `host` when
  // `read`), back = true downloads the block into `host`
  int io(bool back, void* host, void* field, size_t bytes, bool read = false) {
    return back ? down(host, *(void**)field, bytes) : up(field, read ? host : nullptr, bytes);
  }
  int sync() { return rc != FMCMC_OK ? rc : check(hipStreamSynchronize(stream), "hipStreamSynchronize(stream)"); }
};

static void stage_kernel(HostStage& H, const fmcmc_kernel* kn) {
  const size_t kd = sizeof(double) * (size_t)H.k;
  H.up(&H.dk.mu, kn->mu, kd);
  H.up(&H.dk.scale, kn->scale, kd);
  H.up(&H.dk.lb, kn->lb, kd);
  H.up(&H.dk.ub, kn->ub, kd);
  H.up(&H.dk.fixed, kn->fixed, (size_t)H.k);
  if (kn->scheme_seq && kn->scheme_len > 0) H.up(&H.dk.scheme_seq, kn->scheme_seq, sizeof(int32_t) * (size_t)kn->scheme_len);
  if (kn->constr && kn->kind == FMCMC_KERNEL_RAM) H.up(&H.dk.constr, kn->constr, sizeof(double) * (size_t)H.kf * H.kf);
}

// what a run may be fed: the plan of scheme = "random" (in when fed, out otherwise: fetch_call) and the variates
static void stage_run_fed(HostStage& H, const fmcmc_kernel* kn, const fmcmc_run* run, const fmcmc_state* st) {
  const size_t rows = H.C * H.nsteps;
  if (st->scheme_cols) H.up(&H.ds.scheme_cols, st->scheme_cols, sizeof(int32_t) * rows);
  if (run->rng_mode == FMCMC_RNG_FED) {
    H.up(&H.dr.fed_logu, run->fed_logu, sizeof(double) * rows);
    H.up(&H.dr.fed_z, run->fed_z, sizeof(double) * rows * variates_per_step(kn, H.kf));
  }
}

// fmcmc_state in (back = false) or out (back = true).  A fresh state is not read: its blocks are allocated only; f0 is never
// read; nerrors starts from 0 when fresh or when the caller keeps none.
static void io_state(HostStage& H, fmcmc_state* st, bool back) {
  const size_t C = H.C, Ck = sizeof(double) * C * H.k;
  const bool carried = !H.fresh;
  H.io(back, st->theta0, &H.ds.theta0, Ck, true);
  H.io(back, st->f0, &H.ds.f0, sizeof(double) * C);
  if (H.mirror && H.rc == FMCMC_OK) {
    if (!st->mirror_mu || !st->mirror_scale || !st->obs_arate || !st->abs_iter) {
      set_err("mirror kernels need state->mirror_mu, mirror_scale, obs_arate and abs_iter");
      H.rc = FMCMC_ERR_ARG;
      return;
    }
    H.io(back, st->abs_iter, &H.ds.abs_iter, sizeof(int64_t) * C, carried);
    H.io(back, st->mirror_mu, &H.ds.mirror_mu, Ck, carried);
    H.io(back, st->mirror_scale, &H.ds.mirror_scale, Ck, carried);
    H.io(back, st->obs_arate, &H.ds.obs_arate, Ck, carried);
  }
  if (H.adaptive) {
    H.io(back, st->abs_iter, &H.ds.abs_iter, sizeof(int64_t) * C, carried);
    H.io(back, st->Sigma, &H.ds.Sigma, sizeof(double) * C * H.kf * H.kf, carried);
    H.io(back, st->mean_prev, &H.ds.mean_prev, sizeof(double) * C * H.kf, carried);
    H.io(back, st->have_mean, &H.ds.have_mean, sizeof(int32_t) * C, carried);
    if (!back || st->nerrors) H.io(back, st->nerrors, &H.ds.nerrors, sizeof(int32_t) * C, carried && st->nerrors);
    if (!back && !(carried && st->nerrors)) H.fill(H.ds.nerrors, 0, sizeof(int32_t) * C);
  }
}

// fmcmc_out in (blocks only; samples start as NaN, status_theta as 0) or out
static void io_out(HostStage& H, fmcmc_out* out, bool back) {
  const size_t C = H.C, rows = sizeof(double) * C * H.S;
  H.io(back, out->samples, &H.dout.samples, rows * H.k);
  if (!back) H.fill(H.dout.samples, 0xff, rows * H.k);
  if (out->logpost) H.io(back, out->logpost, &H.dout.logpost, rows);
  if (out->draws) H.io(back, out->draws, &H.dout.draws, rows * H.k);
  H.io(back, out->accept_count, &H.dout.accept_count, sizeof(int64_t) * C);
  if (out->accept_bits) H.io(back, out->accept_bits, &H.dout.accept_bits, sizeof(uint32_t) * C * H.nwords);
  H.io(back, out->status, &H.dout.status, sizeof(int32_t) * C);
  H.io(back, out->status_step, &H.dout.status_step, sizeof(int64_t) * C);
  H.io(back, out->status_theta, &H.dout.status_theta, sizeof(double) * C * H.k);
  if (!back) H.fill(H.dout.status_theta, 0, sizeof(double) * C * H.k);
}

// the verdict of a call that ran: FMCMC_ERR_CHAIN with the message of the first chain that stopped
static int report_chain_status(const fmcmc_run* run, const fmcmc_out* out) {
  for (int64_t c = 0; c < run->nchains; c++) {
    if (out->status[c] == FMCMC_CHAIN_OK) continue;
    // NaN log-posterior: the message of R/mcmc.R:759-765; the engine's own conditions by name
    const char* what = "fun(par) is undefined.";
    switch (out->status[c]) {
      case FMCMC_CHAIN_NAN_LOGPOST: what = "fun(par) is undefined (NaN)."; break;
      case FMCMC_CHAIN_NAN_RATIO: what = "fun(par) is undefined (f1 - f0 is NaN)."; break;
      case FMCMC_CHAIN_NOT_PD: what = "'Sigma' is not positive definite."; break;
      case FMCMC_CHAIN_BAD_WINDOW: what = "subscript out of bounds: the rows kernel_adapt(bw / freq) adapts on reach before the first row of this call."; break;
      case FMCMC_CHAIN_SYNC_TIMEOUT: what = "a grid-wide hand-over of the observation-sharded evaluation timed out; the results of this call are invalid (FMCMC_AMD_DEBUG=shard=0 selects the chain-sharded kernel)."; break;
      default: break;
    }
    // (R/mcmc.R:759-765 attaches the fun / lb / ub hint to a NaN log-posterior only)
    const bool nan_status = out->status[c] == FMCMC_CHAIN_NAN_LOGPOST || out->status[c] == FMCMC_CHAIN_NAN_RATIO;
    set_err("%s (chain %lld, status %d).%s This error ocurred during step i = %lld",
            what, (long long)(run->chain_base + c), out->status[c],
            nan_status ? " Check either -fun- or the -lb- and -ub- parameters." : "", (long long)out->status_step[c]);
    return FMCMC_ERR_CHAIN;
  }
  return FMCMC_OK;
}

// Both entry points around their sweep: everything but the model in ...
static void stage_call(HostStage& H, const fmcmc_kernel* kn, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out) {
  stage_kernel(H, kn);
  stage_run_fed(H, kn, run, st);
  io_state(H, st, false);
  io_out(H, out, false);
}
// ... and, where the sweep ran, the state, the plan of scheme = "random" the library drew itself and the outputs back; the
// state counts as carried only after a clean synchronise
static int fetch_call(HostStage& H, const fmcmc_kernel* kn, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out) {
  io_state(H, st, true);
  if (st->scheme_cols && run->rng_mode != FMCMC_RNG_FED && is_simple_kind(kn->kind) && kn->scheme == FMCMC_SCHEME_RANDOM)
    H.down(st->scheme_cols, H.ds.scheme_cols, sizeof(int32_t) * H.C * H.nsteps);
  io_out(H, out, true);
  if (H.sync() != FMCMC_OK) return H.rc;
  st->fresh = 0;
  return report_chain_status(run, out);
}

}  // namespace
