"""Record of profiles/newton_policy_refactor_check.json: the decisions of newton() / group_newton() of one library against another's.

  newton_policy_check.py run OUT.json          (GMPNP_LIB names the library) every case below, per time step: Newton iterations,
                                               krylov_per_iteration[], direct_solves, SHA-256 of the state after the step
  newton_policy_check.py compare A B C [BENCH] A, B: two runs of the parent's library, C: the branch's; prints the table.  BENCH:
                                               lines "<parent|branch> <bench.py's JSON line>" of alternated bench runs

A case counts as reproducible when A and B agree in every recorded figure of every step; the branch is then held to the same."""
import copy, hashlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYS = ("newton", "krylov_per_iteration", "direct_solves", "state_sha256")


def record(run, steps, before_step=None):
    rows = []
    try:
        for k in range(steps):
            if before_step:
                before_step(run, k)
            st = run.step(verbose=False)
            rows.append({"newton": st["iterations"], "krylov_per_iteration": list(st.get("krylov_per_iteration", [])), "krylov": st["krylov_iterations"],
                         "direct_solves": st.get("direct_solves", 0), "state_sha256": hashlib.sha256(run.history[-1].tobytes()).hexdigest()})
    finally:
        run.sys.close()
    return rows


def run_cases(out):
    from gmpnp_amd import backend
    from gmpnp_amd.pore3d import PoreRun, SOLVER_PARAMETERS
    from gmpnp_amd.edl1d import EDLRun
    pore10 = dict(concentration_elec=0.5, L=10e-9, R=5e-9)
    capped = copy.deepcopy(SOLVER_PARAMETERS)
    capped["newton_solver"]["krylov_solver"] = {"maximum_iterations": 3}   # the thin-pore fallback case of tests/test_gpu_parity.py

    def recover(run, k):   # BiCGStab fails for ten steps, then works again: sticky / back-off run out over the rest
        run.solver_parameters = capped if k < 10 else SOLVER_PARAMETERS

    cases = {"pore50_bench_52": lambda: record(PoreRun(num_steps=52, concentration_elec=0.5, L=50e-9, R=5e-9), 52),   # bench.py: 2 warm-up + 50 timed steps
             "pore10_krylov_cap3_fallback_30": lambda: record(PoreRun(num_steps=30, solver_parameters=capped, **pore10), 30),
             "pore10_fallback_then_recover_40": lambda: record(PoreRun(num_steps=40, **pore10), 40, recover),
             "pore10_two_partitions_6": lambda: record(PoreRun(num_steps=6, partition=(2, None), **pore10), 6),
             "pore10_two_partitions_refine1_multilevel_4": lambda: record(PoreRun(num_steps=4, partition=(2, None), refine=1, multilevel=True, **pore10), 4),
             "edl50_100": lambda: record(EDLRun(), 100)}
    for name, opt in (("coarse_refresh_1", dict(coarse_refresh=1)), ("coarse_refresh_3", dict(coarse_refresh=3)), ("warm_start_m1", dict(warm_start=-1)),
                      ("warm_in_stream", dict(warm_in_stream=1)), ("progress_by_copy", dict(progress_by_copy=1)), ("burst_iterations_3", dict(burst_iterations=3)),
                      ("phase_timing", dict(phase_timing=1))):
        cases["pore10_6_" + name] = lambda opt=opt: record(PoreRun(num_steps=6, device_kwargs=opt, **pore10), 6)
    res = {"build_id": backend.load_library().gmpnp_build_id().decode(), "cases": {}}
    for name, fn in cases.items():
        res["cases"][name] = fn()
        print(name, sum(r["newton"] for r in res["cases"][name]), sum(r["krylov"] for r in res["cases"][name]), flush=True)
        with open(out, "w") as fh:
            json.dump(res, fh)


def compare(a, b, c, bench=None):
    A, B, C = (json.load(open(p)) for p in (a, b, c))
    out = {"what": "parent against itself (two processes) and against the branch, per time step: Newton iterations, krylov_per_iteration[], "
                   "direct_solves, SHA-256 of the state; tools/newton_policy_check.py",
           "build_id": {"parent": [A["build_id"], B["build_id"]], "branch": C["build_id"]}, "cases": {}}
    for name, rows in A["cases"].items():
        same = lambda X, k: [r[k] for r in X["cases"][name]] == [r[k] for r in rows]
        out["cases"][name] = {"steps": len(rows), "newton_iterations": sum(r["newton"] for r in rows), "krylov_iterations": sum(r["krylov"] for r in rows),
                              "direct_solves": sum(r["direct_solves"] for r in rows),
                              "parent_reproduces_itself": {k: same(B, k) for k in KEYS}, "branch_equals_parent": {k: same(C, k) for k in KEYS},
                              "per_step": {"newton": [r["newton"] for r in rows], "direct_solves": [r["direct_solves"] for r in rows],
                                           "krylov_per_iteration": [r["krylov_per_iteration"] for r in rows],
                                           "state_sha256_16": [r["state_sha256"][:16] for r in rows]}}
    out["all_bitwise_equal"] = all(all(c["parent_reproduces_itself"].values()) and all(c["branch_equals_parent"].values()) for c in out["cases"].values())
    if bench:
        runs = {"parent": [], "branch": []}
        for line in open(bench):
            who, js = line.split(None, 1)
            runs[who].append(json.loads(js)["value"])
        mp, mb = statistics.median(runs["parent"]), statistics.median(runs["branch"])
        spread = max(runs["parent"]) - min(runs["parent"])
        out["bench"] = {"what": "bench.py --gpus 1 (defaults), parent and branch alternated in one job, Newton iterations/s in run order",
                        "parent": runs["parent"], "branch": runs["branch"], "parent_median": mp, "branch_median": mb,
                        "parent_min_to_max_spread": spread, "branch_median_minus_parent_median": mb - mp, "branch_within_parent_spread": mb >= mp - spread}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    run_cases(sys.argv[2]) if sys.argv[1] == "run" else compare(*sys.argv[2:])
