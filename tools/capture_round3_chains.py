#!/usr/bin/env python3
"""
capture_round3_chains.py — record the round-3 build's chains for test_early_rejection_changes_nothing_observable.

  python tools/capture_round3_chains.py ROUND3_LIB [OUT.npz]     (needs the GPU; OUT defaults to tests/golden/round3_chains.npz)

ROUND3_LIB is the HIP library as committed in round 3 (rsf_build_id() 96c179e837e4be05: no early rejection, tier decided by a
wave's worst lane for the whole solve), built from its own tree:
  git worktree add /tmp/r3 78d7ceb && make -C /tmp/r3/bayesian-markov-chain-monte-carlo_amd/csrc librsf_hip.so

For both problems of the test (headline-like all-TIGHT chains, and the wide-proposal mix) it takes the start state this tree's
library gives, runs the round-3 library from that state, and stores the start state and what the round-3 run returned, kept
small: the accept flags as bits, the sample trace of the chains that stayed finite as its SHA-256 (the test asks for bit
identity), the chains whose sigma^2 went non-finite as bits, and the sigma^2 trace of a fixed sample of STD2_CHAINS chains
(the whole trace is 2 MB of random draws per problem).
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ["RSF_ALLOW_CHECKER_ENGINE"] = "1"

C, ITERS = 8192, 30
STD2_CHAINS = 1024
BUILD_ID = b"96c179e837e4be05"


def problem(engine, oracle_mod, wide):
    """The test's own setup on `engine`, up to the start state (before any set_state from the other build)."""
    from test_gpu_parity import _wide_proposal_problem

    data = _wide_proposal_problem(engine, oracle_mod, C, dc_true=100.0 if wide else 1000.0)
    q0 = np.random.default_rng(3).uniform(60.0, 1500.0, (C, 1)) if wide else np.full((C, 1), 1000.0)
    engine.mcmc_init(q0, data, [0.0], [1e4], seed=4242, prior_len=3)
    if wide:
        st = engine.get_state()
        engine.set_state(V=np.full_like(st[3], 600.0 ** 2))


def q_digest(tq, ok):
    """SHA-256 of the sample trace of the chains in `ok` (float64, C order) → uint8[32]."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(tq[:, ok], dtype=np.float64).tobytes()).digest(), np.uint8)


def std2_chains():
    return np.sort(np.random.default_rng(0).choice(C, STD2_CHAINS, replace=False))


def main():
    import bayesian_markov_chain_monte_carlo_amd as pkg
    import rsf_oracle

    pkg._abi.load()  # loads the one HIP runtime (RTLD_GLOBAL) that both libraries resolve their hip* symbols from
    old = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    for name, (restype, argtypes) in pkg._abi.PROTOTYPES.items():
        if hasattr(old, name):
            getattr(old, name).restype, getattr(old, name).argtypes = restype, argtypes
    assert old.rsf_backend() == b"hip-gfx950" and old.rsf_build_id() == BUILD_ID, old.rsf_build_id()
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "round3_chains.npz")
    rec = {}
    for case, wide in (("tight", False), ("wide", True)):
        with pkg.Engine(mem="host") as e:
            problem(e, rsf_oracle, wide)
            start = [np.array(x) for x in e.get_state()]
        with pkg.Engine(lib=old, mem="host") as e:
            problem(e, rsf_oracle, wide)
            e.set_state(*start)
            tq, ts, ta = (np.array(x) for x in e.mcmc_run(ITERS))
        bugged = ~np.isfinite(ts).all(axis=0)
        for key, v in zip(("q", "ssq", "std2", "V"), start):
            rec[f"{case}_start_{key}"] = v
        rec[f"{case}_accept_bits"] = np.packbits(ta.astype(bool), axis=1)
        rec[f"{case}_nonfinite_bits"] = np.packbits(bugged)
        rec[f"{case}_q_sha256"] = q_digest(tq, ~bugged)
        rec[f"{case}_std2_sample"] = ts[:, std2_chains()]
        print(f"{case}: {ta.astype(bool).mean():.3f} accepted, {bugged.sum()} chains with a non-finite sigma^2")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **rec)
    print(f"wrote {out_path} ({os.path.getsize(out_path)} bytes)")


if __name__ == "__main__":
    main()
