"""ctypes binding of include/fmcmc_amd.h. Fails loudly when the HIP library is missing:
the engine has no CPU fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMCMC_AMD_LIB") or os.path.join(_HERE, "lib", "libfmcmc_amd.so")  # override: A/B builds

_dp = C.POINTER(C.c_double)

FAM_GAUSSIAN_LINREG, FAM_LOGISTIC, FAM_IID_NORMAL = 1, 2, 3
KERNEL_NORMAL, KERNEL_NORMAL_REFLECTIVE, KERNEL_ADAPT, KERNEL_RAM, KERNEL_UNIF, KERNEL_UNIF_REFLECTIVE = 1, 2, 3, 4, 5, 6
RAM_QFUN_T_K, RAM_QFUN_NORMAL, RAM_QFUN_T_DF = 0, 1, 2   # fmcmc_kernel.ram_qfun
KERNEL_NMIRROR, KERNEL_UMIRROR = 7, 8
MIRROR_KERNELS = (KERNEL_NMIRROR, KERNEL_UMIRROR)
SIMPLE_KERNELS = (KERNEL_NORMAL, KERNEL_NORMAL_REFLECTIVE, KERNEL_UNIF, KERNEL_UNIF_REFLECTIVE) + MIRROR_KERNELS
SCHEME_JOINT, SCHEME_ORDERED, SCHEME_RANDOM, SCHEME_EXPLICIT = 0, 1, 2, 3
ABI_VERSION = 6
RNG_PHILOX, RNG_FED = 0, 1
OK, ERR_ARG, ERR_DEVICE, ERR_CHAIN, ERR_UNSUPPORTED, ERR_FUN = 0, 1, 2, 3, 4, 5
CHAIN_OK, CHAIN_NAN_LOGPOST, CHAIN_NAN_RATIO, CHAIN_NOT_PD, CHAIN_BAD_WINDOW, CHAIN_SYNC_TIMEOUT = 0, 1, 2, 3, 4, 5
MAX_K = 256        # (FMCMC_MAX_K; every kernel / option up to MAX_K_WAVE, the joint simple kernels, kernel_adapt and kernel_ram beyond)
MAX_K_WAVE = 64

EXPORTS = ["fmcmc_abi_version", "fmcmc_last_error", "fmcmc_last_kernel", "fmcmc_device_count", "fmcmc_kept_rows",
           "fmcmc_validate", "fmcmc_mcmc_run_dev", "fmcmc_mcmc_run_host", "fmcmc_gelman_partial_len",
           "fmcmc_gelman_work_len",
           "fmcmc_gelman_partial_dev", "fmcmc_gelman_finish", "fmcmc_detmath_dev", "fmcmc_rng_stream_dev",
           "fmcmc_validate_fun", "fmcmc_mcmc_run_fun_dev", "fmcmc_mcmc_run_fun_host",
           "fmcmc_summary_work_len", "fmcmc_summary_pooled_len", "fmcmc_summary_dev",
           "fmcmc_heidel_work_len", "fmcmc_heidel_out_len", "fmcmc_heidel_dev", "fmcmc_plan_route",
           "fmcmc_chain_order_work_len", "fmcmc_chain_order_dev", "fmcmc_raftery_work_len", "fmcmc_raftery_out_len",
           "fmcmc_raftery_dev", "fmcmc_hpd_work_len", "fmcmc_hpd_dev", "fmcmc_autocov_out_len", "fmcmc_autocov_dev",
           "fmcmc_logpost_dev", "fmcmc_validate_user", "fmcmc_mcmc_run_user_dev",
           "fmcmc_validate_batch", "fmcmc_mcmc_run_batch_dev", "fmcmc_mcmc_run_batch_host",
           "fmcmc_mcmc_run_batch_sel_dev", "fmcmc_gelman_groups_work_len", "fmcmc_gelman_groups_dev",
           "fmcmc_summary_groups_work_len", "fmcmc_summary_groups_dev",
           "fmcmc_rank_work_len", "fmcmc_rank_rhat_out_len", "fmcmc_rank_scores_dev", "fmcmc_rank_rhat_dev",
           "fmcmc_rank_ess_work_len", "fmcmc_rank_ess_out_len", "fmcmc_rank_ess_dev",
           "fmcmc_rank_groups_max_values", "fmcmc_rank_rhat_groups_work_len", "fmcmc_rank_rhat_groups_dev",
           "fmcmc_rank_ess_groups_work_len", "fmcmc_rank_ess_groups_out_len", "fmcmc_rank_ess_groups_dev",
           "fmcmc_waic_part_rows", "fmcmc_waic_parts", "fmcmc_waic_work_len", "fmcmc_waic_dev", "fmcmc_waic_groups_dev",
           "fmcmc_loo_tail_len", "fmcmc_loo_plan", "fmcmc_loo_work_len", "fmcmc_loo_state_offset", "fmcmc_loo_dev",
           "fmcmc_loo_groups_dev", "fmcmc_loo_predictive_work_len", "fmcmc_loo_predictive_dev",
           "fmcmc_pointwise_block_rows", "fmcmc_waic_fun_work_len", "fmcmc_waic_fun_dev", "fmcmc_loo_fun_work_len",
           "fmcmc_loo_fun_state_offset", "fmcmc_loo_fun_dev", "fmcmc_predict_work_len", "fmcmc_predict_dev",
           "fmcmc_predictive_work_len", "fmcmc_predictive_dev", "fmcmc_detmath_host",
           "fmcmc_ppc_work_len", "fmcmc_ppc_dev", "fmcmc_ppc_yrep_dev", "fmcmc_ppc_elem_host"]
PPC_MAX_SEL = 65535            # selected draws of one fmcmc_ppc_yrep_dev call
PPC_STATS = ("mean", "sd", "min", "max", "chisq")   # the statistics of fmcmc_ppc_dev's counts, in the order of `total`
PREDICT_LINPRED, PREDICT_EPRED = 0, 1   # fmcmc_predict_dev: kind
LOO_PLAN_LEN = 16              # FMCMC_LOO_PLAN_LEN
BATCH_STREAM_DATA = 1          # fmcmc_mcmc_run_batch_*: flags bit, read the datasets from global memory every step
SUMMARY_MAX_PROBS = 16
CHAIN_ORDER_MAX_RANKS = 2 * SUMMARY_MAX_PROBS
RAFTERY_MAX_THINNINGS = 32     # thinnings per fmcmc_raftery_dev call
HPD_MAX_TAIL = 8192            # rows N - gap of each tail fmcmc_hpd_dev holds in LDS
AUTOCOV_MAX_LAGS = 32          # lags per fmcmc_autocov_dev call

# fmcmc_logpost_fn: out[c] = log f(theta[c][0..k-1]) for c < nchains; 0 = ok (theta, out, hip_stream, user: addresses)
LOGPOST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
# fmcmc_pointwise_fn: ll[b][i] = log p(y_i | theta[b][0..k-1]) for b < B, i < n; 0 = ok (theta, B, k, n, ll, hip_stream, user)
POINTWISE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)


class StepEnv(C.Structure):
    """fmcmc_step_env: what a user-defined kernel's callbacks see of a loop step (device addresses)."""
    _fields_ = [("i", C.c_int64), ("nsteps", C.c_int64), ("nchains", C.c_int64), ("chain_base", C.c_int64),
                ("step_base", C.c_int64), ("k", C.c_int32), ("theta0", C.c_void_p), ("theta1", C.c_void_p),
                ("f0", C.c_void_p), ("f1", C.c_void_p), ("status", C.c_void_p)]


# fmcmc_proposal_fn / fmcmc_logratio_fn: (env, out, hip_stream, user) -> 0 = ok
STEP_FN = C.CFUNCTYPE(C.c_int, C.POINTER(StepEnv), C.c_void_p, C.c_void_p, C.c_void_p)
PROPOSAL_FN = LOGRATIO_FN = STEP_FN


class Model(C.Structure):
    _fields_ = [("family", C.c_int32), ("p", C.c_int32), ("n", C.c_int64), ("X", C.c_void_p),
                ("y", C.c_void_p), ("intercept", C.c_int32), ("guard", C.c_int32),
                ("prior_div", C.c_double)]


class Kernel(C.Structure):
    _fields_ = [("kind", C.c_int32), ("k", C.c_int32), ("mu", C.c_void_p), ("scale", C.c_void_p),
                ("lb", C.c_void_p), ("ub", C.c_void_p), ("fixed", C.c_void_p), ("scheme", C.c_int32),
                ("freq", C.c_int32), ("warmup", C.c_int32), ("bw", C.c_int32), ("until", C.c_double),
                ("eps", C.c_double), ("arate", C.c_double), ("Sd", C.c_double),
                ("scheme_seq", C.c_void_p), ("scheme_len", C.c_int32), ("nadapt", C.c_int32),
                ("constr", C.c_void_p), ("h_fixed", C.c_void_p), ("h_lb", C.c_void_p), ("h_ub", C.c_void_p),
                ("h_scale", C.c_void_p), ("h_scheme_seq", C.c_void_p),
                ("ram_qfun", C.c_int32), ("reserved", C.c_int32), ("ram_df", C.c_double), ("ram_eta_exp", C.c_double)]


class Run(C.Structure):
    _fields_ = [("nchains", C.c_int64), ("nsteps", C.c_int64), ("burnin", C.c_int64),
                ("thin", C.c_int64), ("seed", C.c_uint64), ("chain_base", C.c_int64),
                ("step_base", C.c_int64), ("rng_mode", C.c_int32), ("reserved", C.c_int32),
                ("fed_logu", C.c_void_p), ("fed_z", C.c_void_p)]


class State(C.Structure):
    _fields_ = [("theta0", C.c_void_p), ("f0", C.c_void_p), ("abs_iter", C.c_void_p),
                ("Sigma", C.c_void_p), ("mean_prev", C.c_void_p), ("have_mean", C.c_void_p),
                ("nerrors", C.c_void_p), ("fresh", C.c_int32), ("reserved", C.c_int32),
                ("scheme_cols", C.c_void_p), ("mirror_mu", C.c_void_p), ("mirror_scale", C.c_void_p),
                ("obs_arate", C.c_void_p)]


class Out(C.Structure):
    _fields_ = [("samples", C.c_void_p), ("logpost", C.c_void_p), ("draws", C.c_void_p),
                ("accept_count", C.c_void_p), ("accept_bits", C.c_void_p), ("status", C.c_void_p),
                ("status_step", C.c_void_p), ("status_theta", C.c_void_p), ("ld_rows", C.c_int64)]


_lib = None


def lib():
    """Loads fmcmc_amd/lib/libfmcmc_amd.so (built by fmcmc_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "HIP engine library not found at %s. Build it with `python -m fmcmc_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.fmcmc_abi_version.restype = C.c_int
        if L.fmcmc_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild with "
                               "`python -m fmcmc_amd.build`." % (LIB_PATH, L.fmcmc_abi_version(), ABI_VERSION))
        L.fmcmc_last_error.restype = C.c_char_p
        L.fmcmc_last_kernel.restype = C.c_char_p
        L.fmcmc_device_count.restype = C.c_int
        L.fmcmc_kept_rows.restype = C.c_int64
        L.fmcmc_kept_rows.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        L.fmcmc_validate.restype = C.c_int
        L.fmcmc_validate.argtypes = [C.POINTER(Model), C.POINTER(Kernel), C.POINTER(Run)]
        for nm in ("fmcmc_mcmc_run_dev", "fmcmc_mcmc_run_host"):
            f = getattr(L, nm)
            f.restype = C.c_int
        L.fmcmc_mcmc_run_dev.argtypes = [C.POINTER(Model), C.POINTER(Kernel), C.POINTER(Run),
                                         C.POINTER(State), C.POINTER(Out), C.c_void_p]
        L.fmcmc_mcmc_run_host.argtypes = [C.POINTER(Model), C.POINTER(Kernel), C.POINTER(Run),
                                          C.POINTER(State), C.POINTER(Out), C.c_int]
        L.fmcmc_validate_fun.restype = C.c_int
        L.fmcmc_validate_fun.argtypes = [C.POINTER(Kernel), C.POINTER(Run)]
        L.fmcmc_mcmc_run_fun_dev.restype = C.c_int
        L.fmcmc_mcmc_run_fun_dev.argtypes = [C.POINTER(Kernel), C.POINTER(Run), C.POINTER(State), C.POINTER(Out),
                                             LOGPOST_FN, C.c_void_p, C.c_void_p]
        L.fmcmc_mcmc_run_fun_host.restype = C.c_int
        L.fmcmc_mcmc_run_fun_host.argtypes = [C.POINTER(Kernel), C.POINTER(Run), C.POINTER(State), C.POINTER(Out),
                                              LOGPOST_FN, C.c_void_p, C.c_int]
        L.fmcmc_logpost_dev.restype = C.c_int
        L.fmcmc_logpost_dev.argtypes = [C.POINTER(Model), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.fmcmc_validate_user.restype = C.c_int
        L.fmcmc_validate_user.argtypes = [C.POINTER(Run), C.c_int32]
        L.fmcmc_mcmc_run_user_dev.restype = C.c_int
        L.fmcmc_mcmc_run_user_dev.argtypes = [C.POINTER(Model), LOGPOST_FN, PROPOSAL_FN, LOGRATIO_FN, C.c_void_p, C.c_int32,
                                              C.POINTER(Run), C.POINTER(State), C.POINTER(Out), C.c_void_p]
        L.fmcmc_validate_batch.restype = C.c_int
        L.fmcmc_validate_batch.argtypes = [C.POINTER(Model), C.c_int64, C.POINTER(Kernel), C.POINTER(Run)]
        L.fmcmc_mcmc_run_batch_dev.restype = C.c_int
        L.fmcmc_mcmc_run_batch_dev.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_int64, C.POINTER(Kernel), C.POINTER(Run),
                                               C.POINTER(State), C.POINTER(Out), C.c_uint32, C.c_void_p]
        L.fmcmc_mcmc_run_batch_sel_dev.restype = C.c_int
        L.fmcmc_mcmc_run_batch_sel_dev.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_int64, C.POINTER(Kernel), C.POINTER(Run),
                                                   C.POINTER(State), C.POINTER(Out), C.c_void_p, C.c_uint32, C.c_void_p]
        L.fmcmc_mcmc_run_batch_host.restype = C.c_int
        L.fmcmc_mcmc_run_batch_host.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_int64, C.POINTER(Kernel), C.POINTER(Run),
                                                C.POINTER(State), C.POINTER(Out), C.c_uint32, C.c_int]
        L.fmcmc_gelman_partial_len.restype = C.c_int64
        L.fmcmc_gelman_partial_len.argtypes = [C.c_int32]
        L.fmcmc_gelman_partial_dev.restype = C.c_int
        L.fmcmc_gelman_work_len.restype = C.c_int64
        L.fmcmc_gelman_work_len.argtypes = [C.c_int64, C.c_int32]
        L.fmcmc_gelman_partial_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
                                               C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        L.fmcmc_gelman_groups_work_len.restype = C.c_int64
        L.fmcmc_gelman_groups_work_len.argtypes = [C.c_int64, C.c_int64, C.c_int32]
        L.fmcmc_gelman_groups_dev.restype = C.c_int
        L.fmcmc_gelman_groups_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                              C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_gelman_finish.restype = C.c_int
        L.fmcmc_gelman_finish.argtypes = [_dp, C.c_int32, C.c_int64, _dp, _dp]
        L.fmcmc_summary_work_len.restype = C.c_int64
        L.fmcmc_summary_work_len.argtypes = [C.c_int64, C.c_int32, C.c_int32]
        L.fmcmc_summary_pooled_len.restype = C.c_int64
        L.fmcmc_summary_pooled_len.argtypes = [C.c_int32, C.c_int32]
        L.fmcmc_summary_dev.restype = C.c_int
        L.fmcmc_summary_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_int32, _dp, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_summary_groups_work_len.restype = C.c_int64
        L.fmcmc_summary_groups_work_len.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int32]
        L.fmcmc_summary_groups_dev.restype = C.c_int
        L.fmcmc_summary_groups_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_int32, C.c_void_p, _dp, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        for nm in ("fmcmc_heidel_work_len", "fmcmc_heidel_out_len"):
            getattr(L, nm).restype = C.c_int64
            getattr(L, nm).argtypes = [C.c_int64, C.c_int32, C.c_int64]
        L.fmcmc_heidel_dev.restype = C.c_int
        L.fmcmc_heidel_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                       C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_chain_order_work_len.restype = C.c_int64
        L.fmcmc_chain_order_work_len.argtypes = [C.c_int64, C.c_int32, C.c_int32]
        L.fmcmc_chain_order_dev.restype = C.c_int
        L.fmcmc_chain_order_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                            C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_raftery_work_len.restype = C.c_int64
        L.fmcmc_raftery_work_len.argtypes = [C.c_int64, C.c_int32, C.c_int64]
        L.fmcmc_raftery_out_len.restype = C.c_int64
        L.fmcmc_raftery_out_len.argtypes = [C.c_int64, C.c_int32, C.c_int32]
        L.fmcmc_raftery_dev.restype = C.c_int
        L.fmcmc_raftery_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_int32, C.c_double, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_hpd_work_len.restype = C.c_int64
        L.fmcmc_hpd_work_len.argtypes = [C.c_int64, C.c_int32]
        L.fmcmc_hpd_dev.restype = C.c_int
        L.fmcmc_hpd_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_autocov_out_len.restype = C.c_int64
        L.fmcmc_autocov_out_len.argtypes = [C.c_int64, C.c_int32, C.c_int32]
        L.fmcmc_autocov_dev.restype = C.c_int
        L.fmcmc_autocov_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                        C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_rank_work_len.restype = C.c_int64
        L.fmcmc_rank_work_len.argtypes = [C.c_int64, C.c_int32, C.c_int64]
        L.fmcmc_rank_rhat_out_len.restype = C.c_int64
        L.fmcmc_rank_rhat_out_len.argtypes = [C.c_int64, C.c_int32]
        L.fmcmc_rank_scores_dev.restype = C.c_int
        L.fmcmc_rank_scores_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                            C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_rank_rhat_dev.restype = C.c_int
        L.fmcmc_rank_rhat_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_rank_ess_work_len.restype = C.c_int64
        L.fmcmc_rank_ess_work_len.argtypes = [C.c_int64, C.c_int32, C.c_int64]
        L.fmcmc_rank_ess_out_len.restype = C.c_int64
        L.fmcmc_rank_ess_out_len.argtypes = [C.c_int64, C.c_int32, C.c_int64]
        L.fmcmc_rank_ess_dev.restype = C.c_int
        L.fmcmc_rank_ess_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_rank_groups_max_values.restype = C.c_int64
        L.fmcmc_rank_groups_max_values.argtypes = []
        L.fmcmc_rank_rhat_groups_work_len.restype = C.c_int64
        L.fmcmc_rank_rhat_groups_work_len.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int64]
        L.fmcmc_rank_rhat_groups_dev.restype = C.c_int
        L.fmcmc_rank_rhat_groups_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                                 C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        L.fmcmc_rank_ess_groups_work_len.restype = C.c_int64
        L.fmcmc_rank_ess_groups_work_len.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int64]
        L.fmcmc_rank_ess_groups_out_len.restype = C.c_int64
        L.fmcmc_rank_ess_groups_out_len.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int64]
        L.fmcmc_rank_ess_groups_dev.restype = C.c_int
        L.fmcmc_rank_ess_groups_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                                C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_waic_part_rows.restype = C.c_int64
        L.fmcmc_waic_part_rows.argtypes = []
        L.fmcmc_waic_parts.restype = C.c_int64
        L.fmcmc_waic_parts.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        L.fmcmc_waic_work_len.restype = C.c_int64
        L.fmcmc_waic_work_len.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_int64]
        L.fmcmc_waic_dev.restype = C.c_int
        L.fmcmc_waic_dev.argtypes = [C.POINTER(Model), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_waic_groups_dev.restype = C.c_int
        L.fmcmc_waic_groups_dev.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                            C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]
        L.fmcmc_loo_tail_len.restype = C.c_int64
        L.fmcmc_loo_tail_len.argtypes = [C.c_int64]
        L.fmcmc_loo_plan.restype = C.c_int
        L.fmcmc_loo_plan.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        L.fmcmc_loo_work_len.restype = C.c_int64
        L.fmcmc_loo_work_len.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_int64]
        L.fmcmc_loo_state_offset.restype = C.c_int64
        L.fmcmc_loo_state_offset.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_int64]
        L.fmcmc_loo_dev.restype = C.c_int
        L.fmcmc_loo_dev.argtypes = [C.POINTER(Model), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_loo_groups_dev.restype = C.c_int
        L.fmcmc_loo_groups_dev.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                           C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.fmcmc_loo_predictive_work_len.restype = C.c_int64
        L.fmcmc_loo_predictive_work_len.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64]
        L.fmcmc_loo_predictive_dev.restype = C.c_int
        L.fmcmc_loo_predictive_dev.argtypes = [C.POINTER(Model), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("fmcmc_pointwise_block_rows", "fmcmc_waic_fun_work_len", "fmcmc_loo_fun_work_len",
                     "fmcmc_loo_fun_state_offset"):
            getattr(L, name).restype = C.c_int64
            getattr(L, name).argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64]
        L.fmcmc_waic_fun_dev.restype = C.c_int
        L.fmcmc_waic_fun_dev.argtypes = [POINTWISE_FN, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                         C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_loo_fun_dev.restype = C.c_int
        L.fmcmc_loo_fun_dev.argtypes = [POINTWISE_FN, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                        C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        L.fmcmc_predict_work_len.restype = C.c_int64
        L.fmcmc_predict_work_len.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_int32]
        L.fmcmc_predict_dev.restype = C.c_int
        L.fmcmc_predict_dev.argtypes = [C.POINTER(Model), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                        C.c_int32, _dp, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_predictive_work_len.restype = C.c_int64
        L.fmcmc_predictive_work_len.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64, C.c_int32]
        L.fmcmc_predictive_dev.restype = C.c_int
        L.fmcmc_predictive_dev.argtypes = [C.POINTER(Model), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                           _dp, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_detmath_host.restype = C.c_int
        L.fmcmc_detmath_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
        L.fmcmc_ppc_work_len.restype = C.c_int64
        L.fmcmc_ppc_work_len.argtypes = [C.POINTER(Model), C.c_int64, C.c_int64]
        L.fmcmc_ppc_dev.restype = C.c_int
        L.fmcmc_ppc_dev.argtypes = [C.POINTER(Model), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                    C.c_uint64, C.c_int64, C.c_int64, C.c_int64, _dp, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
        L.fmcmc_ppc_yrep_dev.restype = C.c_int
        L.fmcmc_ppc_yrep_dev.argtypes = [C.POINTER(Model), C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_uint64, C.c_int64,
                                         C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.c_void_p,
                                         C.c_void_p]
        L.fmcmc_ppc_elem_host.restype = C.c_int
        L.fmcmc_ppc_elem_host.argtypes = [C.c_int32, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_double,
                                          C.c_void_p, C.c_void_p]
        L.fmcmc_rng_stream_dev.restype = C.c_int
        L.fmcmc_rng_stream_dev.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                           C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmcmc_detmath_dev.restype = C.c_int
        L.fmcmc_detmath_dev.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p]
        L.fmcmc_plan_route.restype = C.c_int
        L.fmcmc_plan_route.argtypes = [C.POINTER(Model), C.POINTER(Kernel), C.POINTER(Run), C.c_int64, C.c_int32,
                                       C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


def last_error():
    return lib().fmcmc_last_error().decode("utf-8", "replace")


def last_kernel():
    """Kernel variant chosen by this thread's last sweep (diagnostic; results never depend on it)."""
    return lib().fmcmc_last_kernel().decode("utf-8", "replace")


def plan_route(model, kernel, run, ld_rows=0, ncu=256):
    """(code, line): the route planned for a call whose kernel holds HOST pointers, as one line of key=value fields
    (fmcmc_plan_route; no device needed).  A refused call returns fmcmc_validate's code and an empty line."""
    buf = C.create_string_buffer(1024)
    rc = lib().fmcmc_plan_route(C.byref(model), C.byref(kernel), C.byref(run), ld_rows, ncu, buf, len(buf))
    return rc, buf.value.decode("ascii")
