"""Records the SVM solver's answers, to the bit, in train_bits.json next to
this file — run from the repo root on a GPU:

    python tests/golden/make_train_bits.py [--commit ID]

lm_train_solve is a one-problem lm_train_solve_many, so a comparison of the
two says nothing about the solver's arithmetic any more; this fixture does.
It holds what the tree with two separate solvers returned (its "produced_by"
names the commit and the compiler; the build has -ffp-contract=off, so the
bits follow from the order of operations), and tests/test_gpu_train_bits.py
compares with it.  Regenerate it only with a change
that means to move the bits, and say so there.

Only runtime.Trainer's public calls and the sample sets of train_harness.py
and train_cv_harness.py are used.  Per case: the parameters, the sha256 of
the inputs' bytes (a changed generator is told apart from a changed solver),
the sha256 of W's bytes, rho and the stats' floats as float.hex(), the integer
stats, the held-out counts, and for some the sha256 of margins(W, rho)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "train_bits.json")
EPS = 1e-8

# (kh, kw), n as tests/test_gpu_train_cv.py's SINGLE_CASES, the kinds of train_harness.KINDS in turn
SINGLE_CASES = [((1, 1), 1), ((5, 7), 65), ((5, 7), 1023), ((5, 7), 1024), ((5, 7), 1025), ((16, 26), 1000),
                ((24, 24), 1000), ((64, 64), 70)]
MARGINS_AT = (((5, 7), 1025), ((24, 24), 1000))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def encode(res):
    """(W, rho, stats[, heldout]) as the fixture holds it."""
    out = {"W_sha256": sha(np.asarray(res[0], np.float64)), "rho": float(res[1]).hex(),
           "stats": {k: v.hex() if isinstance(v, float) else int(v) for k, v in res[2].items()}}
    if len(res) > 3:
        out["heldout"] = {k: int(v) for k, v in res[3].items()}
    return out


def solve_key(size, n, kind, cp, cn, eps, max_iter):
    return f"{size[0]}x{size[1]} n={n} {kind} c=({cp!r}, {cn!r}) eps={eps!r} max_iter={max_iter}"


def many_key(size, n):
    return f"{size[0]}x{size[1]} n={n} overlapping, company_groups, the 2 PB + 1 list"


def inputs(P, y, groups=None):
    out = {"P_sha256": sha(np.asarray(P, np.uint8)), "y_sha256": sha(np.asarray(y, np.int8))}
    if groups is not None:
        out["groups_sha256"] = sha(np.asarray(groups, np.int32))
    return out


def load():
    with open(FIXTURE) as fh:
        return json.load(fh)


def mismatch(entry, P, y, results, groups=None, z=None):
    """"" when `results` (one (W, rho, stats[, heldout]) per recorded problem)
    and the margins z, if given, are the entry's, else what differs; changed
    inputs are named as such."""
    if entry["inputs"] != inputs(P, y, groups):
        return "the fixture's inputs are not this test's (the sample generator changed, not the solver): " \
               f"{entry['inputs']} recorded, {inputs(P, y, groups)} here"
    got = [encode(r) for r in results]
    if got != entry["results"]:
        return f"the solver's bits moved: recorded {entry['results']}, got {got}"
    if z is not None and entry.get("margins_sha256") != sha(np.asarray(z, np.float64)):
        return f"the margins' bits moved: recorded {entry.get('margins_sha256')}, got {sha(np.asarray(z, np.float64))}"
    return ""


def the_long_list(CV, pb):
    """The 2 PB + 1 problems of CV.company_lists as (c_pos, c_neg, held_out)."""
    lst = [l for l in CV.company_lists(pb) if len(l) == 2 * pb + 1]
    assert len(lst) == 1
    return [(s, s, h) for s, h in lst[0]]


def record():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import train_cv_harness as CV
    import train_harness as TH

    from locomouse_cpp_amd import runtime

    def solve_entry(size, n, kind, cp, cn, eps, max_iter, margins=False):
        P, y = TH.sample_set(kind, n, size[0] * size[1])
        tr = runtime.Trainer(size[0], size[1], n)
        tr.add_patches(P, y)
        res = tr.solve(cp, cn, eps, max_iter)
        e = {"size": list(size), "n": n, "kind": kind, "c_pos": cp, "c_neg": cn, "eps": eps, "max_iter": max_iter,
             "inputs": inputs(P, y), "results": [encode(res)]}
        if margins:
            e["margins_sha256"] = sha(tr.margins(res[0], res[1]))
        tr.close()
        return solve_key(size, n, kind, cp, cn, eps, max_iter), e

    solve = {}
    for i, (size, n) in enumerate(SINGLE_CASES):
        kind = TH.KINDS[i % len(TH.KINDS)]
        k, e = solve_entry(size, n, kind, *TH.kind_costs(kind), EPS, 200, margins=(size, n) in MARGINS_AT)
        solve[k] = e
    # tests/test_gpu_train.py's own case at (5 x 7, 1025), and test_costs_kind_with_its_costs
    for size, n, m in (((5, 7), 1025, True), ((5, 7), 300, False)):
        k, e = solve_entry(size, n, "costs", 10.0, 1.0, EPS, 200, margins=m)
        solve[k] = e
    for max_iter in (1, 0):  # test_max_iter_returns_ok_unconverged
        k, e = solve_entry((5, 7), 200, "overlapping", 1.0, 1.0, 1e-12, max_iter)
        solve[k] = e
    many = {}
    for size, n in CV.COMPANY_CASES:
        P, y = TH.sample_set("overlapping", n, size[0] * size[1])
        groups = CV.company_groups(n)
        tr = runtime.Trainer(size[0], size[1], n + 17)
        tr.add_patches(P, y)
        tr.set_groups(groups)
        pb = tr.problem_block()
        problems = the_long_list(CV, pb)
        res = list(zip(*tr.solve_many(problems, EPS, 200)))
        tr.close()
        many[many_key(size, n)] = {"size": list(size), "n": n, "kind": "overlapping", "problem_block": pb,
                                   "problems": [list(p) for p in problems], "eps": EPS, "max_iter": 200,
                                   "inputs": inputs(P, y, groups), "results": [encode(r) for r in res]}
    return solve, many


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit of the tree this runs on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    hipcc = subprocess.check_output(["hipcc", "--version"], text=True).strip().splitlines()[:2]  # HIP and clang versions
    solve, many = record()
    with open(args.out, "w") as fh:
        json.dump({"produced_by": {"commit": commit, "hipcc_version": hipcc,
                                   "command": "python tests/golden/make_train_bits.py"},
                   "solve": solve, "solve_many": many}, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out, len(solve), "solve cases,", len(many), "solve_many calls")


if __name__ == "__main__":
    main()
