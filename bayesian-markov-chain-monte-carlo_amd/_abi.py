"""
ctypes binding of include/rsf_abi.h.

The product loads exactly one library through this module: csrc/librsf_hip.so (hand-written
gfx950 kernels).  There is no CPU fallback: if the library is missing, cannot be loaded, or no
GPU is visible, `load()` raises.  `bind()` only attaches prototypes to an already opened
library handle, so the test-suite can type the oracle library with the same declarations.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_uint8, c_uint32, c_uint64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
# RSF_HIP_LIB: alternative build of the same HIP library (kernel A/B experiments); never a CPU library
LIB_PATH = os.environ.get("RSF_HIP_LIB") or os.path.join(HERE, "csrc", "librsf_hip.so")

ABI_VERSION = 1
OK = 0
MEM_HOST, MEM_DEVICE = 0, 1
FLAG_RADIATION_DAMPING = 1
FLAG_FP32_SOLVE = 2
FLAG_DOP853 = 4
ADAPT_NONE, ADAPT_REFERENCE_DICT, ADAPT_AM = 0, 1, 2
ADAPT_MODES = {"none": ADAPT_NONE, "reference_dict": ADAPT_REFERENCE_DICT, "am": ADAPT_AM}
MAX_PARAMS = 3
ERR_NOT_POSDEF = -6
# rsf_mcmc_counters: index = RSF_CNT_* of include/rsf_abi.h
COUNTERS = ("accepted", "evaluated", "nonfinite", "out_of_bounds", "early_rejected", "wave_solves", "wave_skips",
            "steps_tight", "steps_narrow", "steps_wide", "steps_full", "steps_redone", "lane_steps", "steps_unguarded")


class RsfError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"rsf error {code}: {message}")
        self.code = code


class Config(ctypes.Structure):
    _fields_ = [
        ("size", c_uint32),
        ("version", c_uint32),
        ("device", c_int32),
        ("mem_space", c_int32),
        ("stream", c_void_p),
        ("block_threads", c_uint32),
        ("cpu_threads", c_uint32),
    ]


class Model(ctypes.Structure):
    _fields_ = [
        ("size", c_uint32),
        ("flags", c_uint32),
        ("nsteps", c_int32),
        ("substeps", c_int32),
        ("t_start", c_double),
        ("t_final", c_double),
        ("mu_ref", c_double),
        ("V_ref", c_double),
        ("k1", c_double),
        ("mu_t_zero", c_double),
        ("a", c_double),
        ("b", c_double),
    ]


class McmcConfig(ctypes.Structure):
    _fields_ = [
        ("size", c_uint32),
        ("n_params", c_int32),
        ("n_chains", c_int64),
        ("chain_offset", c_int64),
        ("seed", c_uint64),
        ("n0", c_double),
        ("prior_len", c_int32),
        ("adapt_mode", c_int32),
        ("adapt_interval", c_int32),
        ("n_groups", c_int32),
        ("fd_rel_step", c_double),
        ("lo", c_double * MAX_PARAMS),
        ("hi", c_double * MAX_PARAMS),
    ]


_P = c_void_p  # array arguments travel as raw addresses (host ndarray or device tensor)

PROTOTYPES = {
    "rsf_version": (c_int, []),
    "rsf_backend": (c_char_p, []),
    "rsf_build_id": (c_char_p, []),
    "rsf_last_error": (c_char_p, []),
    "rsf_device_count": (c_int, []),
    "rsf_create": (c_int, [POINTER(Config), POINTER(c_void_p)]),
    "rsf_destroy": (c_int, [c_void_p]),
    "rsf_sync": (c_int, [c_void_p]),
    "rsf_set_model": (c_int, [c_void_p, POINTER(Model)]),
    "rsf_model_nout": (c_int, [c_void_p, POINTER(c_int32)]),
    "rsf_forward_batch": (c_int, [c_void_p, c_int64, _P, _P, _P, _P, _P, _P]),
    "rsf_mcmc_init": (c_int, [c_void_p, POINTER(McmcConfig), _P, _P]),
    "rsf_mcmc_get_state": (c_int, [c_void_p, _P, _P, _P, _P]),
    "rsf_mcmc_set_state": (c_int, [c_void_p, _P, _P, _P, _P]),
    "rsf_mcmc_run": (c_int, [c_void_p, c_int64, _P, _P, _P]),
    "rsf_mcmc_replay": (c_int, [c_void_p, c_int64, _P, _P, _P, _P, _P, _P]),
    "rsf_mcmc_stats": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "rsf_mcmc_counters": (c_int, [c_void_p, POINTER(c_int64), c_int32]),
    "rsf_mcmc_init_state": (c_int, [c_void_p, POINTER(McmcConfig), _P, _P, _P, _P]),
    "rsf_mcmc_propose": (c_int, [c_void_p, _P, _P, _P]),
    "rsf_mcmc_replay_ssq": (c_int, [c_void_p, c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "rsf_pool_summary": (c_int, [c_void_p, c_int64, _P, c_int64, POINTER(c_double)]),
    "rsf_pool_kde": (c_int, [c_void_p, c_int64, _P, c_int64, c_int32, _P, c_double, _P]),
    "rsf_pool_histogram": (c_int, [c_void_p, c_int64, _P, c_int64, c_int32, c_double, c_double, _P]),
    "rsf_comm_unique_id": (c_int, [POINTER(c_uint8)]),
    "rsf_comm_init": (c_int, [c_void_p, c_int32, c_int32, POINTER(c_uint8)]),
    "rsf_comm_destroy": (c_int, [c_void_p]),
    "rsf_pool_allgather": (c_int, [c_void_p, _P, c_int64, _P]),
    "rsf_pool_allreduce_sum": (c_int, [c_void_p, _P, c_int64]),
    "rsf_comm_init_all": (c_int, [POINTER(c_void_p), c_int32]),
    "rsf_pool_allgather_all": (c_int, [POINTER(c_void_p), c_int32, POINTER(c_void_p), c_int64, POINTER(c_void_p)]),
    "rsf_pool_allreduce_sum_all": (c_int, [POINTER(c_void_p), c_int32, POINTER(c_void_p), c_int64]),
    "rsf_philox4x32_10": (c_int, [POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "rsf_mcmc_adapt": (c_int, [c_int32, c_int32, _P, c_int32, c_int32, _P]),
    "rsf_mcmc_draws": (c_int, [c_uint64, c_int64, c_int64, c_int32, c_double, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
}


# include/rsf_diag.h: exported by librsf_hip.so only (the CPU checker implements rsf_abi.h alone), bound by load()
DIAG_PROTOTYPES = {
    "rsf_diag_partials": (c_int, [c_void_p, c_int64, c_int64, c_int32, _P, c_int64, POINTER(c_double), c_int64, c_int64,
                                  POINTER(c_double)]),
    "rsf_diag_finish": (c_int, [c_int64, c_int32, c_int64, POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_double)]),
    "rsf_diag_rank_prepare": (c_int, [c_void_p, c_int64, c_int64, c_int32, _P, c_int32, POINTER(c_double), c_double,
                                      POINTER(c_double), _P]),
    "rsf_diag_rank_partials": (c_int, [c_void_p, c_int64, c_int64, POINTER(c_double)]),
    "rsf_diag_rank_finish": (c_int, [c_int64, c_int32, POINTER(c_double), c_int32, POINTER(c_double), c_int64, POINTER(c_double)]),
    "rsf_diag_rank_release": (c_int, [c_void_p]),
}
DIAG_HEAD = 9  # RSF_DIAG_HEAD: fields of the partials before the lag sums
# rsf_diag_finish out[p][RSF_DIAG_OUT], in index order
DIAG_OUT = ("mean", "var_plus", "W", "B_over_N", "split_rhat", "nested_rhat", "K", "ess", "tau", "mcse_mean", "lags_complete")
# rank-normalised diagnostics (rsf_diag_rank_*): the four derived series, prepare's stats[p][DIAG_RANK_STATS + n_probs] in index order
# (then the n_probs quantiles) and rsf_diag_rank_finish out[p][RSF_DIAG_RANK_OUT] in index order
DIAG_RANK_SERIES = ("bulk", "folded", "q05", "q95")
DIAG_RANK_STATS = ("median", "q05", "q95", "hdi_lo", "hdi_hi", "nonfinite", "const_bulk", "const_folded", "const_q05", "const_q95")
DIAG_RANK_OUT = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "lags_complete")


# include/rsf_predict.h: posterior predictive checks; exported by librsf_hip.so only, bound by load()
PREDICT_PROTOTYPES = {
    "rsf_predict_partials": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, POINTER(c_double), POINTER(c_double), POINTER(c_double), _P]),
    "rsf_predict_finish": (c_int, [c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double),
                                   POINTER(c_double)]),
    "rsf_predict_quantiles": (c_int, [c_void_p, c_int64, c_int64, _P, c_int32, POINTER(c_double), POINTER(c_double)]),
}
PREDICT_HEAD = 2  # RSF_PREDICT_HEAD: n, sum of sigma^2
# the partials' fields per output time (RSF_PREDICT_FIELDS), rsf_predict_finish's out_rows and out_totals, in index order
PREDICT_FIELDS = ("sum_y", "sum_y2", "sum_l", "sum_l2", "sum_exp", "sum_phi", "nonfinite")
PREDICT_OUT = ("mean", "var", "pit", "lpd", "p_waic_k")
PREDICT_TOTALS = ("mean_std2", "elpd_waic", "p_waic", "elpd_waic_se")
PREDICT_MAX_PROBS = 16  # RSF_PREDICT_MAX_PROBS: probabilities per rsf_predict_quantiles call


# include/rsf_psis.h: PSIS-LOO on the predictive series; exported by librsf_hip.so only, bound by load()
PSIS_PROTOTYPES = {
    "rsf_predict_psis_loo": (c_int, [c_void_p, c_int64, c_int64, _P, _P, _P, c_double, POINTER(c_double)]),
    "rsf_predict_psis_finish": (c_int, [c_int64, c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
}
# rsf_predict_psis_loo's out_rows and rsf_predict_psis_finish's out_totals, in index order
PSIS_OUT = ("elpd_loo_k", "pareto_k", "n_tail", "weight_ess")
PSIS_TOTALS = ("elpd_loo", "p_loo", "elpd_loo_se", "k_threshold", "n_high_k", "max_pareto_k")
PSIS_MAX_TAIL = 8192  # RSF_PSIS_MAX_TAIL: largest ceil(min(0.2 n, 3 sqrt(n / r_eff)))


# include/rsf_predict_noise.h: the predictive band that includes the noise; exported by librsf_hip.so only, bound by load()
PREDICT_NOISE_PROTOTYPES = {
    "rsf_predict_noise_quantiles": (c_int, [c_void_p, c_int64, c_int64, _P, _P, c_int32, POINTER(c_double), POINTER(c_double),
                                            POINTER(c_int32)]),
}
PREDICT_NOISE_MAX_PASSES = 129  # RSF_PREDICT_NOISE_MAX_PASSES: pass 0, at most 64 bisections and 64 Newton steps


# include/rsf_joint.h: the joint posterior of the pooled draws; exported by librsf_hip.so only, bound by load()
JOINT_PROTOTYPES = {
    "rsf_pool_joint_partials": (c_int, [c_void_p, c_int64, c_int32, _P, POINTER(c_double), POINTER(c_double)]),
    "rsf_pool_joint_finish": (c_int, [c_int32, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "rsf_pool_kde2d": (c_int, [c_void_p, c_int64, c_int32, _P, c_int32, c_int32, c_int32, _P, c_double, POINTER(c_double), c_int64, _P]),
    "rsf_pool_histogram2d": (c_int, [c_void_p, c_int64, c_int32, _P, c_int32, c_int32, c_int32, c_double, c_double, c_int32, c_double,
                                     c_double, _P]),
    "rsf_pool_hpd_levels": (c_int, [c_int64, POINTER(c_double), c_int32, POINTER(c_double), POINTER(c_double)]),
}
JOINT_HEAD = 2  # RSF_JOINT_HEAD: n_finite, nonfinite; then d sums and d (d + 1) / 2 sums of products (upper triangle, row-major)
JOINT_MAX_PARAMS = 8  # RSF_JOINT_MAX_PARAMS
HIST2D_MAX_CELLS = 16384  # RSF_HIST2D_MAX_CELLS: (nbx + 2) (nby + 2)
JOINT_OUT = ("mean", "cov", "corr")  # rsf_pool_joint_finish's out: d, d * d and d * d doubles (RSF_JOINT_OUT(d) in all)


# include/rsf_evidence.h: the marginal likelihood of the pooled draws by bridge sampling; exported by librsf_hip.so only, bound by load()
EVIDENCE_PROTOTYPES = {
    "rsf_evidence_propose": (c_int, [c_void_p, c_int64, c_int32, POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_double),
                                     POINTER(c_double), c_uint64, c_int64, _P, _P, _P]),
    "rsf_evidence_logg": (c_int, [c_void_p, c_int64, c_int32, _P, POINTER(c_double), POINTER(c_double), POINTER(c_int32), _P]),
    "rsf_evidence_logtarget": (c_int, [c_void_p, c_int64, c_int32, _P, _P, c_double, POINTER(c_double), POINTER(c_double), POINTER(c_int32),
                                       _P, _P]),
    "rsf_evidence_partials": (c_int, [c_void_p, c_int64, _P, c_int64, _P, c_double, c_double, c_double, c_double, POINTER(c_double)]),
    "rsf_evidence_finish": (c_int, [POINTER(c_double), c_double, c_double, c_double, c_double, c_int32, POINTER(c_double), POINTER(c_double),
                                    POINTER(c_double)]),
}
EVIDENCE_MAX_PARAMS = 3  # RSF_EVIDENCE_MAX_PARAMS
# rsf_evidence_partials' partials and rsf_evidence_finish's out, in index order
EVIDENCE_PARTIALS = ("n1", "n2", "n2_finite", "sum_num", "sum_den", "sum_f1", "sum_f1_sq", "sum_f2", "sum_f2_sq")
EVIDENCE_OUT = ("r_next", "log_integral", "log_evidence", "re")
EVIDENCE_MAX_ITER = 1000  # Engine.evidence_bridge: iterations at most
EVIDENCE_RTOL = 1e-10     # ... and the relative change of r below which it has converged


# include/rsf_smc.h: tempered sequential Monte Carlo over the box prior; exported by librsf_hip.so only, bound by load()
SMC_PROTOTYPES = {
    "rsf_smc_init": (c_int, [c_void_p, c_int64, c_int32, POINTER(c_double), POINTER(c_double), c_uint64, c_int64, _P]),
    "rsf_smc_weight_sums": (c_int, [c_void_p, c_int64, _P, c_int32, POINTER(c_double), c_double, POINTER(c_double)]),
    "rsf_smc_section": (c_int, [c_double, c_int32, POINTER(c_double), POINTER(c_int32)]),
    "rsf_smc_increment": (c_int, [c_int64, c_double, c_double, c_double, POINTER(c_double)]),
    "rsf_smc_log_evidence": (c_int, [c_double, c_double, c_int32, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "rsf_smc_resample": (c_int, [c_void_p, c_int64, c_int32, _P, _P, c_double, c_double, c_double, _P, _P, _P, _P]),
    "rsf_smc_move": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, c_double, POINTER(c_double), POINTER(c_double), POINTER(c_double),
                             c_double, c_uint64, c_int64, c_int64, c_int32, POINTER(c_int64)]),
    "rsf_smc_move_propose": (c_int, [c_void_p, c_int64, c_int32, _P, POINTER(c_double), POINTER(c_double), POINTER(c_double), c_uint64,
                                     c_int64, c_int64, _P, _P]),
    "rsf_smc_move_accept": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, _P, _P, c_double, c_double, c_uint64, c_int64, c_int64,
                                    POINTER(c_int64)]),
    "rsf_smc_std2": (c_int, [c_void_p, c_int64, _P, c_double, c_uint64, c_int64, c_int64, _P]),
}
SMC_MAX_PARAMS = 3       # RSF_SMC_MAX_PARAMS
SMC_MAX_CANDIDATES = 16  # RSF_SMC_MAX_CANDIDATES: steps evaluated in one read of l, the sections of Engine.smc's search
SMC_HEAD = 3             # RSF_SMC_HEAD: lmax, finite entries, -inf entries before rsf_smc_weight_sums' sums
SMC_MAX_STEPS = 64       # RSF_SMC_MAX_STEPS
SMC_ROUNDS = 6           # Engine.smc: rounds of the 16-section search for the next temperature step
SMC_RESAMPLE_COUNTER = (0xFFFFFFFF, 0xFFFFFFFF, 4)  # Philox counter (particle lo, particle hi, ., slot) of a stage's resampling uniform


# include/rsf_smc_batch.h: P independent SMC populations per call; exported by librsf_hip.so only, bound by load().  The
# per-population parameter arrays are host arrays and travel as typed pointers, the particles as raw addresses
_U64P, _I64P, _I32P, _U8P, _DP = POINTER(c_uint64), POINTER(c_int64), POINTER(c_int32), POINTER(c_uint8), POINTER(c_double)
SMC_BATCH_PROTOTYPES = {
    "rsf_smc_batch_init": (c_int, [c_void_p, c_int32, c_int64, c_int32, _DP, _DP, _U64P, _I64P, _P]),
    "rsf_smc_batch_logtarget": (c_int, [c_void_p, c_int32, c_int64, c_int32, _P, _P, c_int32, _I32P, c_double, _DP, _DP, _P]),
    "rsf_smc_batch_weight_sums": (c_int, [c_void_p, c_int32, c_int64, _P, c_int32, _DP, _DP, _U8P, _DP]),
    "rsf_smc_batch_resample": (c_int, [c_void_p, c_int32, c_int64, c_int32, _P, _P, _DP, _DP, _DP, _U8P, _P, _P, _P, _P]),
    "rsf_smc_batch_move": (c_int, [c_void_p, c_int32, c_int64, c_int32, _P, _P, _P, c_int32, _I32P, c_double, _DP, _DP, _DP, _DP, _U64P, _I64P,
                                   _I64P, c_int32, _U8P, _I64P]),
    "rsf_smc_batch_std2": (c_int, [c_void_p, c_int32, c_int64, _P, c_double, _U64P, _I64P, _I64P, _P]),
}
SMC_BATCH_MAX = 64  # RSF_SMC_BATCH_MAX: populations per call


# include/rsf_fit.h: multi-start Levenberg-Marquardt least squares; exported by librsf_hip.so only, bound by load()
FIT_PROTOTYPES = {
    "rsf_fit_normal": (c_int, [c_void_p, c_int64, c_int32, _P, _P, c_int32, c_double, _P, _P, _P]),
    "rsf_fit_run": (c_int, [c_void_p, c_int64, c_int32, _P, _P, c_int32, _DP, _DP, c_double, c_double, c_int32, _P, _P, _P, _P, _P, _P]),
    "rsf_fit_trial": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, _P, _DP, _DP, _P, _P, _P]),
    "rsf_fit_decide": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_double]),
    "rsf_fit_laplace": (c_int, [c_int32, c_int64, c_double, c_double, _DP, _DP, _DP, _DP]),
}
FIT_MAX_PARAMS = 3  # RSF_FIT_MAX_PARAMS
FIT_MAX_ITER = 64   # RSF_FIT_MAX_ITER: iterations per rsf_fit_run call
FIT_RUNNING, FIT_CONVERGED, FIT_STALLED, FIT_FAILED = 0, 1, 2, 3  # RSF_FIT_*: a start's status
FIT_LAM0 = 1e-3     # RSF_FIT_LAM0: the damping a start begins with

# include/rsf_mala.h: Gauss-Newton manifold MALA; exported by librsf_hip.so only, bound by load()
MALA_PROTOTYPES = {
    "rsf_mala_run": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, _P, _P, c_int32, _DP, _DP, c_double, c_double, c_double, c_double, c_uint64,
                             c_int64, c_int64, c_int32, _P, _P, _P, _P, _P]),
    "rsf_mala_propose": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, _P, _DP, _DP, c_double, c_double, c_double, c_uint64, c_int64, c_int64,
                                 _P, _P, _P]),
    "rsf_mala_accept": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, _P, _DP, _DP, c_double, c_double, c_double, c_uint64, c_int64, c_int64,
                                _P, _P, _P, _P, _P, _P, _P, _P]),
}
MALA_MAX_PARAMS = 3  # RSF_MALA_MAX_PARAMS
MALA_MAX_ITER = 64   # RSF_MALA_MAX_ITER: iterations per rsf_mala_run call
# include/rsf_ensemble.h: the affine-invariant stretch move in island ensembles; exported by librsf_hip.so only, bound by load()
ENSEMBLE_PROTOTYPES = {
    "rsf_ensemble_run": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, c_int32, _DP, _DP, c_double, c_uint32, c_double, c_uint64, c_int64, c_int64,
                                 c_int32, _P, _P, _P, _P, _P]),
    "rsf_ensemble_propose": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _DP, _DP, c_double, c_uint32, c_uint64, c_int64, c_int64, c_int32, _P, _P, _P]),
    "rsf_ensemble_accept": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _DP, _DP, c_double, c_uint64, c_int64, c_int64, c_int32, _P, _P, _P, _P,
                                    _P, _P, _P]),
    "rsf_ensemble_ssq": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, c_int32, c_int32, _P]),
}
ENSEMBLE_MAX_PARAMS = 3  # RSF_ENSEMBLE_MAX_PARAMS
ENSEMBLE_MAX_ITER = 64   # RSF_ENSEMBLE_MAX_ITER: iterations per rsf_ensemble_run call
# include/rsf_dr.h: two-stage delayed-rejection Metropolis; exported by librsf_hip.so only, bound by load()
DR_PROTOTYPES = {
    "rsf_dr_run": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, c_int32, _DP, _DP, _DP, c_double, c_int32, c_double, c_uint64, c_int64, c_int64,
                           c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "rsf_dr_propose": (c_int, [c_void_p, c_int64, c_int32, _P, _P, c_int32, _DP, _DP, _DP, c_double, c_int32, c_uint64, c_int64, c_int64, _P, _P, _P]),
    "rsf_dr_accept": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _DP, _DP, c_double, c_int32, c_double, c_uint64, c_int64, c_int64, _P, _P, _P, _P,
                              _P, _P, _P, _P, _P, _P]),
    "rsf_dr_ssq": (c_int, [c_void_p, c_int64, c_int32, _P, _P, _P, c_int32, _P]),
}
DR_MAX_PARAMS = 3   # RSF_DR_MAX_PARAMS
DR_MAX_ITER = 64    # RSF_DR_MAX_ITER: iterations per rsf_dr_run call
DR_MAX_GROUPS = 64  # RSF_DR_MAX_GROUPS: observation series, and factors, per call
# include/rsf_grid.h: the exact posterior on a tensor quadrature grid; exported by librsf_hip.so only, bound by load()
GRID_PROTOTYPES = {
    "rsf_grid_logtarget": (c_int, [c_void_p, c_int32, _I32P, _DP, _P, c_double, _DP, _DP, c_int32, _P, _P]),
    "rsf_grid_columns": (c_int, [c_void_p, c_int32, _I32P, _DP, _DP, _P, _P, c_double, _DP, _P, _P, _P]),
    "rsf_grid_finish": (c_int, [c_int32, _I32P, _DP, _DP, c_int32, c_double, c_double, _DP, _DP, c_double, _DP, _DP, _DP, _DP, _DP, _DP, _DP]),
    "rsf_grid_draw": (c_int, [c_void_p, c_int32, _I32P, _DP, c_int32, _P, _DP, _DP, c_uint64, c_int64, c_int64, _P, _P]),
    "rsf_grid_cdf": (c_int, [c_void_p, c_int32, _I32P, _DP, c_int32, _P, _DP, c_int64, _DP, _DP]),
}
GRID_MAX_PARAMS = 3  # RSF_GRID_MAX_PARAMS
GRID_PLAIN, GRID_PRODUCT = 0, 1  # RSF_GRID_PLAIN, RSF_GRID_PRODUCT
GRID_COORDS = {"plain": GRID_PLAIN, "product": GRID_PRODUCT}
# the fields of a column (RSF_GRID_FIELDS) and rsf_grid_finish's head (RSF_GRID_HEAD entries: mean is 3, cov 3 x 3), in index order
GRID_FIELDS = ("s0", "s1", "s2", "ssq", "ssq2", "n_neginf")
GRID_HEAD = 20
GRID_HEAD_SCALARS = {"Z": 0, "log_integral": 1, "log_evidence": 2, "n_neginf": 3, "x0_mean": 16, "x0_var": 17, "std2_mean": 18, "std2_var": 19}
# include/rsf_law.h: the caller's loading history and the state law; exported by librsf_hip.so only, bound by load()
LAW_PROTOTYPES = {
    "rsf_set_loading": (c_int, [c_void_p, _DP, c_int64]),
    "rsf_get_loading": (c_int, [c_void_p, _DP, c_int64]),
    "rsf_loading_size": (c_int, [c_void_p, _I64P]),
    "rsf_law_forward": (c_int, [c_void_p, c_int32, c_int64, _P, _P, _P, _P, _P, _P]),
}
LAW_AGEING, LAW_SLIP = 0, 1  # RSF_LAW_AGEING, RSF_LAW_SLIP
LAWS = {"aging": LAW_AGEING, "ageing": LAW_AGEING, "slip": LAW_SLIP}
# include/rsf_observe.h: the observable of the state-law solve; exported by librsf_hip.so only, bound by load()
OBSERVE_PROTOTYPES = {
    "rsf_law_observe": (c_int, [c_void_p, c_int32, c_int32, c_int64, _P, _P, _P, _P, _P, _P]),
}
OBS_ACC, OBS_MU, OBS_THETA, OBS_VELOCITY = 0, 1, 2, 3  # RSF_OBS_ACC, RSF_OBS_MU, RSF_OBS_THETA, RSF_OBS_VELOCITY
OBSERVABLES = {"acc": OBS_ACC, "mu": OBS_MU, "friction": OBS_MU, "theta": OBS_THETA, "state": OBS_THETA, "velocity": OBS_VELOCITY, "V": OBS_VELOCITY}
# include/rsf_law_dr.h: the delayed-rejection sampler under either state law and any observable; exported by librsf_hip.so only, bound
# by load().  rsf_dr_run's and rsf_dr_ssq's arguments behind (ctx, law, observable)
LAW_DR_PROTOTYPES = {
    "rsf_law_dr_run": (c_int, [c_void_p, c_int32, c_int32] + DR_PROTOTYPES["rsf_dr_run"][1][1:]),
    "rsf_law_dr_ssq": (c_int, [c_void_p, c_int32, c_int32] + DR_PROTOTYPES["rsf_dr_ssq"][1][1:]),
}
# include/rsf_stiff.h: the state-law solve and its delayed-rejection sampler with the spring's stiffness independent of Dc; exported
# by librsf_hip.so only, bound by load().  rsf_law_observe's, rsf_law_dr_run's and rsf_law_dr_ssq's arguments with the stiffness
# behind (ctx, law, observable)
STIFF_PROTOTYPES = {
    "rsf_stiff_observe": (c_int, [c_void_p, c_int32, c_int32, c_double] + OBSERVE_PROTOTYPES["rsf_law_observe"][1][3:]),
    "rsf_stiff_dr_run": (c_int, [c_void_p, c_int32, c_int32, c_double] + DR_PROTOTYPES["rsf_dr_run"][1][1:]),
    "rsf_stiff_dr_ssq": (c_int, [c_void_p, c_int32, c_int32, c_double] + DR_PROTOTYPES["rsf_dr_ssq"][1][1:]),
}
# include/rsf_kstiff.h: the delayed-rejection sampler of the state-law solve with the stiffness among the parameters, the last of
# d = 2 (Dc, k) or 4 (Dc, a, b, k) coordinates; exported by librsf_hip.so only, bound by load().  rsf_stiff_observe's arguments with
# the stiffness an array behind b, rsf_law_dr_run's and rsf_law_dr_ssq's as they are, rsf_dr_propose's and rsf_dr_accept's
KSTIFF_PROTOTYPES = {
    "rsf_kstiff_observe": (c_int, OBSERVE_PROTOTYPES["rsf_law_observe"][1][:7] + [_P] + OBSERVE_PROTOTYPES["rsf_law_observe"][1][7:]),
    "rsf_kstiff_dr_run": (c_int, list(LAW_DR_PROTOTYPES["rsf_law_dr_run"][1])),
    "rsf_kstiff_dr_ssq": (c_int, list(LAW_DR_PROTOTYPES["rsf_law_dr_ssq"][1])),
    "rsf_kstiff_dr_propose": (c_int, list(DR_PROTOTYPES["rsf_dr_propose"][1])),
    "rsf_kstiff_dr_accept": (c_int, list(DR_PROTOTYPES["rsf_dr_accept"][1])),
}
KSTIFF_MAX_PARAMS = 4  # RSF_KSTIFF_MAX_PARAMS
# include/rsf_law_fit.h: the Levenberg-Marquardt fit under either state law and any observable; exported by librsf_hip.so only, bound by
# load().  rsf_fit_normal's and rsf_fit_run's arguments behind (ctx, law, observable)
LAW_FIT_PROTOTYPES = {
    "rsf_law_fit_normal": (c_int, [c_void_p, c_int32, c_int32] + FIT_PROTOTYPES["rsf_fit_normal"][1][1:]),
    "rsf_law_fit_run": (c_int, [c_void_p, c_int32, c_int32] + FIT_PROTOTYPES["rsf_fit_run"][1][1:]),
}
# include/rsf_law_predict.h: the posterior predictive checks under either state law and any observable, and the partials of a series
# that exists; exported by librsf_hip.so only, bound by load().  rsf_predict_partials' arguments behind (ctx, law, observable)
LAW_PREDICT_PROTOTYPES = {
    "rsf_law_predict_partials": (c_int, [c_void_p, c_int32, c_int32] + PREDICT_PROTOTYPES["rsf_predict_partials"][1][1:]),
    "rsf_predict_series_partials": (c_int, [c_void_p, c_int64, c_int64, _P, _P, _P, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
}
# include/rsf_law_grid.h: the exact posterior of a state-law model on a tensor grid in the coordinates of a fit; exported by
# librsf_hip.so only, bound by load()
LAW_GRID_PROTOTYPES = {
    "rsf_law_logtarget": (c_int, [c_void_p, c_int32, c_int32, c_int32, _I32P, _DP, _DP, _DP, _I32P, _I32P, c_int64, _P, _P, _P, c_double, _DP, _DP,
                                  _P, _P, _P]),
    "rsf_law_grid_moments": (c_int, [c_void_p, c_int32, _I32P, _DP, _DP, _DP, _DP, _I32P, _I32P, _P, _P, c_double, _DP, _P, _DP]),
}
LAW_GRID_MAX_PARAMS = 3  # RSF_LAW_GRID_MAX_PARAMS
# the totals of rsf_law_grid_moments (RSF_LAW_GRID_FIELDS), in index order; d0..d2: q - center of (Dc, a, b)
LAW_GRID_FIELDS = ("s0", "d0", "d1", "d2", "d0d0", "d0d1", "d0d2", "d1d1", "d1d2", "d2d2", "ssq", "ssq2")
MAX_BLOCK = 256     # kMaxBlock: a workgroup's threads unless Engine(block_threads=...) says otherwise


def bind(lib):
    """Attach the rsf_abi.h prototypes to an opened CDLL; raises if a symbol is missing."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError names the missing symbol
        fn.restype, fn.argtypes = restype, argtypes
    return lib


_lib = None


def hip_runtime_path():
    """The ONE HIP runtime this process uses.  librsf_hip.so is linked without a runtime dependency
    because two HIP/HSA runtimes in a process cannot both own the GPU: PyTorch's ROCm wheel bundles
    its own libamdhip64.so (no SONAME, so the loader does not unify it with /opt/rocm's), and the
    engine shares device memory and streams with torch.  Order: $RSF_HIP_RUNTIME, torch's bundled
    runtime, then $ROCM_PATH or /opt/rocm."""
    env = os.environ.get("RSF_HIP_RUNTIME")
    if env:
        return env
    try:
        import torch

        cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            return cand
    except ImportError:
        pass
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "lib", "libamdhip64.so")):
            return os.path.join(root, "lib", "libamdhip64.so")
    raise RsfError(-2, "no HIP runtime (libamdhip64.so) found; set RSF_HIP_RUNTIME")


def load():
    """The product library (HIP).  Fails loudly; never substitutes a CPU implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RsfError(-2, f"{LIB_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        ctypes.CDLL(hip_runtime_path(), mode=ctypes.RTLD_GLOBAL)  # resolves the library's hip* symbols
        lib = bind(ctypes.CDLL(LIB_PATH))
        for table in (DIAG_PROTOTYPES, PREDICT_PROTOTYPES, PSIS_PROTOTYPES, PREDICT_NOISE_PROTOTYPES, JOINT_PROTOTYPES, EVIDENCE_PROTOTYPES,
                      SMC_PROTOTYPES, SMC_BATCH_PROTOTYPES, FIT_PROTOTYPES, MALA_PROTOTYPES, ENSEMBLE_PROTOTYPES, GRID_PROTOTYPES,
                      DR_PROTOTYPES, LAW_PROTOTYPES, OBSERVE_PROTOTYPES, LAW_DR_PROTOTYPES, LAW_PREDICT_PROTOTYPES, LAW_FIT_PROTOTYPES,
                      LAW_GRID_PROTOTYPES, STIFF_PROTOTYPES, KSTIFF_PROTOTYPES):
            for name, (restype, argtypes) in table.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
        if lib.rsf_version() != ABI_VERSION:
            raise RsfError(-1, f"ABI version mismatch: library {lib.rsf_version()}, binding {ABI_VERSION}")
        _lib = lib
    return _lib


def check(lib, status):
    if status != OK:
        raise RsfError(status, lib.rsf_last_error().decode("utf-8", "replace"))


def require_device(lib):
    n = lib.rsf_device_count()
    if n <= 0:
        raise RsfError(-2, "no HIP device visible (rsf_device_count() = %d): %s; there is no CPU fallback"
                       % (n, lib.rsf_last_error().decode("utf-8", "replace")))
    return n
