"""fmcmc_amd: MI355X-native many-chain Metropolis-Hastings engine, a drop-in for the hot path of
USCbiostats/fmcmc (MCMC(), kernel_*(), convergence_gelman()).  See DESIGN.md / INTEGRATION.md."""
from .kernels import (kernel_normal, kernel_normal_reflective, kernel_adapt, kernel_am, kernel_ram, kernel_unif,
                      kernel_unif_reflective, kernel_nmirror, kernel_umirror, fmcmc_kernel, plan_update_sequence, check_dimensions, process_bounds,
                      eta_power, qfun_t, qfun_normal, kernel_new)
from .models import gaussian_linreg, logistic, iid_normal, LogPosterior, batched_fun, BatchedFun, model_batch, ModelBatch, pointwise_fun, PointwiseFun
from .mcmc import (MCMC, MCMC_without_conv_checker, MCMC_with_conv_checker, Mcmc, McmcList, check_initial,
                   append_chains, get_logpost, get_draws, get_elapsed, shard_bounds, DeviceChains, get_, get_initial,
                   get_fun, get_nsteps, get_seed, get_nchains, get_burnin, get_thin, get_kernel, get_multicore,
                   get_conv_checker, get_cl, get_progress, get_chain_id, MCMC_OUTPUT, MCMC_batch, McmcBatch, bulk_plan)
from .convergence import (convergence_gelman, convergence_geweke, convergence_heildel, convergence_auto, geweke_diag,
                          heidel_diag, raftery_diag, spectrum0_ar, convergence_rhat, rhat_host, ess_host)
from .recursive import cov_recursive, mean_recursive, reflect_on_boundaries
from .summary import (summary, effective_size, McmcSummary, heidel, HeidelDiag, gelman_diag, GelmanDiag, raftery, RafteryDiag,
                      chain_quantiles, hpd_interval, HpdInterval, autocorr_diag, AutocorrDiag, crosscorr, GelmanDiagBatch,
                      McmcSummaryBatch, summary_batch, rhat, RhatDiag, rank_scores, ess, EssDiag, geyer_tau, rhat_batch,
                      RhatDiagBatch, ess_batch, EssDiagBatch, waic, waic_batch, waic_compare, waic_host, WaicResult, WaicBatch,
                      loo, loo_batch, loo_compare, loo_host, loo_plan, LooResult, LooBatch, waic_host_matrix,
                      loo_host_matrix, waic_loglik, predict, predict_host, PredictResult, predictive, predictive_host,
                      PredictiveResult, loo_predictive, loo_predictive_host, loo_predictive_host_matrix, LooPredictiveResult,
                      ppc, ppc_host, PpcResult, posterior_predict, posterior_predict_selection)

__all__ = ["ppc", "ppc_host", "PpcResult", "posterior_predict", "posterior_predict_selection", "loo_predictive", "loo_predictive_host", "loo_predictive_host_matrix", "LooPredictiveResult", "predictive", "predictive_host", "PredictiveResult", "predict", "predict_host", "PredictResult", "pointwise_fun", "PointwiseFun", "waic_host_matrix", "loo_host_matrix", "waic_loglik", "loo", "loo_batch", "loo_compare", "loo_host", "loo_plan", "LooResult", "LooBatch", "waic", "waic_batch", "waic_compare", "waic_host", "WaicResult", "WaicBatch", "ess_batch", "EssDiagBatch", "rhat_batch", "RhatDiagBatch", "ess", "EssDiag", "ess_host", "geyer_tau", "rhat", "RhatDiag", "rank_scores", "convergence_rhat", "rhat_host", "MCMC_batch", "McmcBatch", "GelmanDiagBatch", "McmcSummaryBatch", "summary_batch", "bulk_plan", "model_batch", "ModelBatch", "hpd_interval", "HpdInterval", "autocorr_diag", "AutocorrDiag", "crosscorr", "raftery", "raftery_diag", "RafteryDiag", "chain_quantiles", "summary", "effective_size", "McmcSummary", "heidel", "HeidelDiag", "gelman_diag", "GelmanDiag", "MCMC", "MCMC_without_conv_checker", "MCMC_with_conv_checker", "kernel_normal",
           "kernel_normal_reflective", "kernel_adapt", "kernel_am", "kernel_ram", "kernel_unif",
           "kernel_unif_reflective", "kernel_nmirror", "kernel_umirror", "gaussian_linreg",
           "logistic", "iid_normal", "batched_fun", "BatchedFun", "convergence_gelman", "convergence_geweke", "convergence_heildel", "convergence_auto",
           "geweke_diag", "heidel_diag", "spectrum0_ar", "Mcmc", "McmcList", "check_initial",
           "append_chains", "get_logpost", "get_draws", "get_elapsed", "shard_bounds", "cov_recursive", "mean_recursive",
           "reflect_on_boundaries", "plan_update_sequence", "get_", "get_initial", "get_fun", "get_nsteps", "get_seed",
           "get_nchains", "get_burnin", "get_thin", "get_kernel", "get_multicore", "get_conv_checker", "get_cl", "get_progress",
           "get_chain_id", "MCMC_OUTPUT", "eta_power", "qfun_t", "qfun_normal", "kernel_new"]
