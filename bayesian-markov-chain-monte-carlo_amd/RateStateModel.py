"""
RateStateModel — drop-in for the reference class of the same name (RateStateModel.py:15-395).

Same constructor, same public attributes, same `evaluate() -> (t, acc, acc_noise)`; the forward
solve runs on the GPU through the C ABI (rsf_forward_batch) as a fixed-step RK4 integration
(`substeps` steps per output interval) instead of the reference's SciPy dop853 call.  DESIGN.md
states the resulting tolerance ladder against the reference trajectory.

Additive surface: `substeps`, `precision`, `integrator`, `loading`, `state_law`, `observable`, `noise_sd`, `stiffness`,
`evaluate_batch(dc, a=None, b=None)`, `trajectory(dc=None, a=None, b=None)`.
"""
import zlib

import numpy as np

if __package__:
    from .engine import Engine, check_law_options, observable_of
else:  # flat layout: this directory on sys.path, the reference's own import style (main.py:44-46)
    from engine import Engine, check_law_options, observable_of

# RateStateModel.py:5-11
A = 0.011
B = 0.014
MU_REF = 0.6
V_REF = 1.0
K1 = 1.0e-7
START_TIME = 0.0
END_TIME = 50.0


def _scalar(x):
    """`model.Dc` may be a Python float or a 1-element array (MCMC.py:381 assigns q_new[0,])."""
    return float(np.asarray(x, dtype=np.float64).reshape(-1)[0])


class RateStateModel:
    def __init__(self, number_time_steps=500, start_time=START_TIME, end_time=END_TIME):
        self.a = A
        self.b = B
        self.mu_ref = MU_REF
        self.V_ref = V_REF
        self.k1 = K1
        self.t_start = start_time
        self.t_final = end_time
        self.num_tsteps = number_time_steps
        self.delta_t = (end_time - start_time) / number_time_steps
        self.mu_t_zero = MU_REF
        self.RadiationDamping = True
        self.Dc = None
        self.substeps = 1  # RK4 steps per delta_t (additive knob; 1 = BASELINE's "fixed-step RK4 nsteps")
        self.precision = "float64"  # additive: "float32" integrates the ODE in single precision (tolerance sweeps)
        self.integrator = "rk4"     # additive: "dop853" = the reference's own adaptive scheme (scipy ode, rtol 1e-6, atol 1e-10)
        # additive: the loading history V_l(t) — None (the reference's V_ref (1 + exp(-t/20) sin 10t)), a callable t -> V_l
        # (vectorised over the RK4 stage times) or an array of one value per stage time (Engine.loading_times()) — and the
        # state evolution law, "aging" (the reference's; "ageing" is accepted) or "slip".  float64 RK4 only
        self.loading = None
        self.state_law = "aging"
        # additive: the series evaluate() returns and the samplers fit — "acc" (the reference's acceleration), "mu" (or "friction":
        # what a laboratory records), "theta" (or "state") or "velocity" (or "V") — and, for the observables other than "acc", the
        # standard deviation of evaluate()'s additive noise (the reference's |acc| N(0, 1) would bury a friction of 0.6 under 0.6).
        # Another observable than "acc" runs the plain float64 RK4 (Engine.law_observe) under either law
        self.observable = "acc"
        self.noise_sd = 0.0
        # additive: the stiffness of the spring — None (the reference's coupling to the parameter being inferred,
        # k' = 1e-2 * 10 / Dc, RateStateModel.py:324) or a positive float, a constant of the apparatus that does not move with Dc.
        # With one, every solve is Engine.law_observe's (rsf_stiff_observe) under either law, for every observable; float64 RK4 only
        self.stiffness = None
        self._engine = None
        self._engine_key = None

    # ---- engine plumbing ----------------------------------------------------------------
    def _loading_key(self):
        """what re-arms the engine when the loading changes: a callable by identity, an array by its values"""
        if self.loading is None or callable(self.loading):
            return self.loading if self.loading is None else id(self.loading)
        v = np.ascontiguousarray(np.asarray(self.loading, dtype=np.float64))
        return (v.shape, zlib.crc32(v.tobytes()))

    def _model_key(self):
        return (self.a, self.b, self.mu_ref, self.V_ref, self.k1, self.t_start, self.t_final, self.num_tsteps, self.delta_t,
                self.mu_t_zero, bool(self.RadiationDamping), int(self.substeps), self.precision, self.integrator, self._loading_key(),
                self.state_law, self.observable, self.stiffness)

    def engine(self):
        """Host-memory Engine bound to the HIP library, re-armed when an attribute changed."""
        if self._engine is None:
            self._engine = Engine(mem="host")
        key = self._model_key()
        if key != self._engine_key:
            self._engine.set_model(self, self.substeps)
            self._engine_key = key
        return self._engine

    def num_outputs(self):
        return int(np.floor((self.t_final - self.t_start) / self.delta_t))  # RateStateModel.py:358

    def time_axis(self):
        """t[k] accumulated the way the reference stores r.t (RateStateModel.py:382-384)."""
        n = self.num_outputs()
        t = np.empty(n)
        t[0] = self.t_start
        for k in range(1, n):
            t[k] = t[k - 1] + self.delta_t
        return t

    # ---- reference surface --------------------------------------------------------------
    def evaluate(self):
        """→ (t, acc, acc_noise); acc_noise = acc + |acc|·N(0,1) from the global NumPy RNG
        (RateStateModel.py:392), so a seeded caller sees the reference's draw order.  With another `observable` than "acc":
        (t, series, series + noise_sd·N(0,1)) from the same RNG."""
        if self.Dc is None:
            raise ValueError("RateStateModel.Dc must be set before evaluate()")
        _, acc = self._forward([_scalar(self.Dc)])
        acc = np.ascontiguousarray(acc[:, 0])
        if observable_of(self) != "acc":  # the chosen series + noise_sd N(0, 1); no variate is drawn at noise_sd = 0
            sd = float(self.noise_sd)
            noisy = acc + sd * np.random.randn(acc.shape[0]) if sd != 0.0 else acc.copy()
            return self.time_axis(), acc, noisy
        acc_noise = acc + 1.0 * np.abs(acc) * np.random.randn(acc.shape[0])
        return self.time_axis(), acc, acc_noise

    # ---- batched surface (additive) -----------------------------------------------------
    def evaluate_batch(self, dc, a=None, b=None):
        """The clean series (the acceleration, or the model's observable) for C parameter sets in one launch → ndarray (C, nout)."""
        _, acc = self._forward(np.asarray(dc, dtype=np.float64).reshape(-1), a=a, b=b)
        return np.ascontiguousarray(acc.T)

    def _forward(self, dc, a=None, b=None):
        """the clean series under the model's loading history and state law: the tier kernels (rsf_forward_batch) for the ageing
        law, the plain float64 RK4 of rsf_law_forward for the slip law; the model's observable, if it is not the acceleration, by
        rsf_law_observe under either law; with a stiffness every observable by rsf_stiff_observe (law_observe routes there)"""
        law = check_law_options(self)
        if observable_of(self) != "acc" or self.stiffness is not None:
            return self.engine().law_observe(law, self.observable, dc, a=a, b=b, want_series=True)
        if law == "slip":
            return self.engine().law_forward("slip", dc, a=a, b=b, want_acc=True)
        return self.engine().forward(dc, a=a, b=b, want_acc=True)

    def trajectory(self, dc=None, a=None, b=None):
        """The four clean series of the state-law solve under the model's loading history and state law → dict(acc, mu, theta,
        velocity), each (nout,) for a scalar dc (None: the model's Dc) or (C, nout) for C parameter sets: one Engine.law_observe
        call each, whatever the model's own observable."""
        law = check_law_options(self)
        if dc is None and self.Dc is None:
            raise ValueError("RateStateModel.Dc must be set before trajectory()")
        one = dc is None or np.ndim(dc) == 0
        q = np.asarray([_scalar(self.Dc if dc is None else dc)] if one else dc, dtype=np.float64).reshape(-1)
        eng, out = self.engine(), {}
        for name in ("acc", "mu", "theta", "velocity"):
            series = np.asarray(eng.law_observe(law, name, q, a=a, b=b, want_series=True)[1])
            out[name] = np.ascontiguousarray(series[:, 0] if one else series.T)
        return out
