"""Greedy versus optimal event matching, on the CPU.

    python scripts/sed_greedy_vs_optimal.py [--rows 20000] [--seed 0]

The event-based counts of metrics.SedEval match greedily: reference events in time order, each taking the earliest free predicted
event within both collars.  sed_eval's default resolves the same compatibility graph with an optimal bipartite matching.  This
script draws random (reference, prediction) rows - a third with long events, a third with short events packed within a collar of
each other, a third with a prediction that is the reference jittered by up to a collar - counts the matches of the definition
(tests/sedeval_ref.greedy_matches) and of scipy.sparse.csgraph.maximum_bipartite_matching on the same graph, and prints how many
rows differ and by how much."""
import argparse
import os
import sys

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import sedeval_ref as R  # noqa: E402

HOP, COLLAR, PCT = 256, 3200, 50


def random_row(rng, kind, t=400):
    if kind == 0:     # long events: block activity in 10 .. 40-frame units
        unit = int(rng.integers(10, 41))
        ref = np.repeat(rng.random(t // unit + 1) < 0.4, unit)[:t]
        pred = np.roll(ref, int(rng.integers(-15, 16))) ^ (rng.random(t) < 0.02)
    elif kind == 1:   # short events, several within a collar (12.5 frames) of each other
        ref = rng.random(t) < rng.choice([0.2, 0.4, 0.6])
        pred = rng.random(t) < rng.choice([0.2, 0.4, 0.6])
    else:             # the reference with every event's ends moved by up to a collar and a half
        ref = np.repeat(rng.random(t // 8 + 1) < 0.35, 8)[:t]
        pred = np.zeros(t, bool)
        for s, e in R.runs(list(ref)):
            s2, e2 = s + int(rng.integers(-18, 19)), e + int(rng.integers(-18, 19))
            pred[max(0, s2):max(0, e2 + 1)] = True
    return R.runs(list(ref)), R.runs(list(pred))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    differ = [0, 0, 0]
    gap = greedy_total = optimal_total = edges = used = 0
    for i in range(args.rows):
        ref, pred = random_row(rng, i % 3)
        if not ref or not pred:
            continue
        used += 1
        graph = np.array([[R.may_match(p, r, HOP, COLLAR, PCT) for p in pred] for r in ref], dtype=np.int8)
        edges += int(graph.sum())
        optimal = int((maximum_bipartite_matching(csr_matrix(graph), perm_type='column') >= 0).sum())
        greedy = R.greedy_matches(ref, pred, HOP, COLLAR, PCT)
        assert greedy <= optimal, (ref, pred)
        greedy_total += greedy
        optimal_total += optimal
        if greedy != optimal:
            differ[i % 3] += 1
            gap += optimal - greedy
    print(f"{used} rows with events on both sides ({args.rows} drawn, seed {args.seed}), {edges} compatible pairs")
    print(f"matches: greedy {greedy_total}, optimal {optimal_total}")
    print(f"rows where greedy < optimal: {sum(differ)} (long events {differ[0]}, packed short events {differ[1]}, jittered {differ[2]}); "
          f"matches lost in all: {gap}")


if __name__ == "__main__":
    main()
