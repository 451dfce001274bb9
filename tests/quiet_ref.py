"""The float64 definition of the noise covariance from the frames outside events that `transforms.quiet_mask`,
`transforms.quiet_ranges`, `FrontendPlan.whiten_factors_ranges` and the kernel k_whiten_factors<true> of k_whiten.h are held to -
NumPy, frame by frame, written independently of the vectorised host code.

    mask[b, t] = 1 for every frame inside any event (sample, first, last; inclusive) of sample b, widened by `guard` frames a
        side and clipped to the sample's own T_b frames
    blocks of `block` frames from frame 0; for block j of sample b and r = 0 .. reach, the first r for which the frames
        [max((j - r) block, 0), min((j + r + 1) block, T_b)) hold at least `min_quiet` unmasked frames: that range, use_mask = 1;
        none: the block's own frames, use_mask = 0 (a block past the sample's end: its own padding frames, use_mask = 0)
    factors: whiten_ref.factors_ref's r00, r11, r10 -> (a, b, c) with the means over the frames of the range that count - the
        unmasked ones (use_mask = 1) or all (use_mask = 0); use_mask = 1 without an unmasked frame: a = b = c = 0
"""
import numpy as np

import extract_ref as X
import whiten_ref as W


def mask_ref(events, n_frames, guard=0):
    """uint8 [B, max T_b]; n_frames: the frame count of every sample."""
    lens = [int(n) for n in n_frames]
    mask = np.zeros((len(lens), max(lens)), np.uint8)
    for s, first, last in np.asarray(events, np.int64).reshape(-1, 3):
        for t in range(int(first) - guard, int(last) + guard + 1):
            if 0 <= t < lens[s]:
                mask[s, t] = 1
    return mask


def ranges_ref(mask, n_frames, block=None, min_quiet=32, reach=1):
    """(ranges int32 [B, J, 3] = (t0, t1, use_mask), quiet int64 [B, J]): counted frame by frame."""
    mask = np.asarray(mask)
    bsz, t = mask.shape
    block, n_blocks = W.block_of(t, block)
    ranges, quiet = np.zeros((bsz, n_blocks, 3), np.int32), np.zeros((bsz, n_blocks), np.int64)
    for b in range(bsz):
        t_b = int(n_frames[b])
        for j in range(n_blocks):
            if j * block >= t_b:
                ranges[b, j] = (j * block, min((j + 1) * block, t), 0)
                continue
            ranges[b, j] = (j * block, min((j + 1) * block, t_b), 0)
            for r in range(reach + 1):
                frames = [u for u in range((j - r) * block, (j + r + 1) * block) if 0 <= u < t_b]
                n = sum(1 for u in frames if not mask[b, u])
                if n >= min_quiet:
                    ranges[b, j], quiet[b, j] = (frames[0], frames[-1] + 1, 1), n
                    break
    return ranges, quiet


def counted_frames(mask, row, b):
    """The frames behind one table row (t0, t1, use_mask) of sample b."""
    t0, t1, use_mask = (int(v) for v in row)
    return [t for t in range(t0, t1) if not (use_mask and mask[b, t])]


def factors_ref(spec, mask, ranges, loading=1e-2):
    """[B, F, T, 4], mask [B, T], ranges [B, J, 3] -> (a [B, F, J], b [B, F, J], c [B, F, J] complex), float64."""
    x = np.asarray(spec, np.float64)
    bsz, f = x.shape[:2]
    n_blocks = ranges.shape[1]
    a, b, c = np.zeros((bsz, f, n_blocks)), np.zeros((bsz, f, n_blocks)), np.zeros((bsz, f, n_blocks), np.complex128)
    for i in range(bsz):
        for j in range(n_blocks):
            frames = counted_frames(mask, ranges[i, j], i)
            if frames:
                one = W.factors_ref(x[i:i + 1][:, :, frames], None, loading)     # the counted frames as one block
                a[i, :, j], b[i, :, j], c[i, :, j] = one[0][0, :, 0], one[1][0, :, 0], one[2][0, :, 0]
    return a, b, c


def quiet_frames_ref(events, quiet, block):
    return np.asarray([min(quiet[s, j] for j in range(first // block, last // block + 1))
                       for s, first, last in np.asarray(events, np.int64).reshape(-1, 3)], np.int64)


# ---------------------------------------------------------------------------
# the demonstration: a dominant event, steered 1/8 sample off
# ---------------------------------------------------------------------------
# (F, T, block, event frames, k_lo): extract_ref's two scenes with the event long enough to dominate its block
SCENES = {"large": (257, 512, None, (56, 455), 8), "small": (33, 96, 32, (20, 75), 2)}
TRUE_DELAY, STEER_ERROR, GUARD = -3.0, 0.125, 2


def scene(which, seed, source_db):
    """(source, noise) of extract_ref.scene_parts, float64 [1, F, T, 4] each, with the scene's (block, frames, k_lo)."""
    f, t, block, frames, k_lo = SCENES[which]
    source, noise = X.scene_parts(seed, f, t, source_delay=TRUE_DELAY, source_db=source_db, frames=frames)
    return source, noise, block, frames, k_lo


def quiet_inputs(t, block, frames, min_quiet, reach):
    """The mask (the event with guard 2) and the range table of a one-sample scene."""
    mask = mask_ref([[0, frames[0], frames[1]]], [t], GUARD)
    return mask, ranges_ref(mask, [t], block, min_quiet, reach)[0]


def gain_of(source, noise, abc, block, frames, k_lo):
    """SINR gain in dB over the event's frames of the beamformer steered STEER_ERROR off, its weights from `abc`."""
    ev, d = [[0, frames[0], frames[1]]], [TRUE_DELAY + STEER_ERROR]
    (ys,), (yn,) = X.beamform_ref(source, ev, d, abc, block), X.beamform_ref(noise, ev, d, abc, block)
    return X.gains(source, noise, ys, yn, frames, k_lo)[0]
