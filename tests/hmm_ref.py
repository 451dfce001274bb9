"""An independent restatement of the HMM event decoder's steps 2-4 in Python integers, written from the definition in
include/iris_frontend.h (iris_decode_events_hmm) and not from challenge_amd/detect.py, and a brute-force maximiser for short
sequences.  Step 1 (the overlap-add average p) is decode_core.h's and is taken as given: these functions start from p."""
import itertools
import math
import struct

N_BUCKETS = 1024
NAN_SCORE = -(1 << 20)
START = -(1 << 60)


def default_lut():
    """lut[i] = rint(256 ln(c / (1 - c))), c = (i + 0.5) / 1024 (Python floats are float64; round() is half to even, as rint)."""
    out = []
    for i in range(N_BUCKETS):
        c = (i + 0.5) / N_BUCKETS
        out.append(int(round(256.0 * math.log(c / (1.0 - c)))))
    return out


def f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def bias_of(threshold):
    t = f32(threshold)
    return int(round(256.0 * math.log(t / (1.0 - t))))


def cost_of(nats):
    return int(round(256.0 * nats))


def score(p, lut, bias):
    """Step 2 for one fp32 value p (given as a Python float holding that value)."""
    if p != p:
        return NAN_SCORE
    x = p * 1024.0               # a power of two: the fp32 product is this value, or overflows to +-inf, which clamps alike
    if x <= 0.0:
        b = 0
    elif x >= 1023.0:
        b = 1023
    else:
        b = int(math.floor(x))
    return int(lut[b]) - bias


def viterbi(e, cost):
    """Step 3 on a list of integer scores: the list s of 0 / 1."""
    n = len(e)
    if n == 0:
        return []
    v0, v1 = 0, START
    b0, b1 = [], []
    for t in range(n):
        b0.append(1 if v1 > v0 else 0)
        b1.append(0 if v0 - cost > v1 else 1)
        v0, v1 = max(v0, v1), e[t] + max(v1, v0 - cost)
    s = [0] * n
    s[n - 1] = 1 if v1 > v0 else 0
    for t in range(n - 1, 0, -1):
        s[t - 1] = b1[t] if s[t] else b0[t]
    return s


def runs(s):
    """Step 4: the maximal runs of ones as [first, last] pairs."""
    out, start = [], None
    for t, v in enumerate(s):
        if v and start is None:
            start = t
        if not v and start is not None:
            out.append([start, t - 1])
            start = None
    if start is not None:
        out.append([start, len(s) - 1])
    return out


def objective(e, s, cost):
    return sum(x for x, on in zip(e, s) if on) - cost * len(runs(s))


def brute_force_best(e, cost):
    """The largest objective over all 2^T paths (T <= 10)."""
    assert len(e) <= 10
    return max(objective(e, s, cost) for s in itertools.product((0, 1), repeat=len(e)))


def decode(p_rows, lut, threshold, cost_nats):
    """Steps 2-4 for one (file, class): the fp32 values p[t] (as Python floats) -> [[first, last], ...]."""
    bias, cost = bias_of(threshold), cost_of(cost_nats)
    return runs(viterbi([score(p, lut, bias) for p in p_rows], cost))
