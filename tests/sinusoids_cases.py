"""The inputs of tests/test_gpu_sinusoids.py, built without a GPU so that tests/test_sinusoids_host.py can hold the reference's
bounds of exactly these cases against the tightness cap."""
import numpy as np

SR = 16000
# B, T, K, hop
SHAPES = [(1, 1, 1, 8), (2, 3, 5, 7), (2, 4, 3, 1), (1, 5, 4, 2), (2, 9, 33, 64), (1, 20, 100, 128), (1, 3, 2, 1024)]
TRACKS = ("random", "octaves", "nyquist", "silent")
LARGE_PHASE = (1, 64, 2, 1024)


def make_case(shape, track, seed, normalize=True):
    B, T, K, hop = shape
    rng = np.random.default_rng(seed)
    f = rng.uniform(50.0, 7000.0, (B, T, K))
    c = rng.uniform(0.05, 2.0, (B, T, K))
    a = rng.uniform(0.1, 1.5, (B, T, 1))
    if track == "octaves":              # neighbouring frames at least an octave apart: what a wrong head, e or segment total would move
        base = rng.uniform(100.0, 1500.0, (B, 1, K))
        up = rng.uniform(2.0, 4.0, (B, T, K))
        f = np.where((np.arange(T) % 2 == 0)[None, :, None], base, base * up)
    elif track == "nyquist":            # tracks that cross sample_rate / 2: masked on some frames only.  The lower half of the
        # partials stays below: a frame with ONE audible partial has a normalised weight of 1 and a grad_c of 0 by cancellation
        f = rng.uniform(6500.0, 9500.0, (B, T, K))               # (in no order: an audible frame follows a masked one)
        f[:, :, :K // 2] = rng.uniform(200.0, 2000.0, (B, T, K // 2))
    elif track == "silent":             # an all-masked frame and a frame whose c is all zero
        f[:, T // 2] = rng.uniform(8001.0, 12000.0, (B, K))
        if T >= 3:
            c[:, T - 1] = 0.0
    return dict(shape=shape, track=track, normalize=normalize, f=f.astype(np.float32), c=c.astype(np.float32), a=a.astype(np.float32))


def forward_cases():
    """every (shape, track) with normalisation, and the random and Nyquist tracks without"""
    out = []
    for i, shape in enumerate(SHAPES):
        for j, track in enumerate(TRACKS):
            out.append(make_case(shape, track, 100 + 10 * i + j, True))
        out.append(make_case(shape, "random", 200 + i, False))
        out.append(make_case(shape, "nyquist", 300 + i, False))
    return out


def large_phase_case():
    """T = 64 frames of hop 1024, a partial just under Nyquist: P reaches 3 10^4 turns"""
    B, T, K, hop = LARGE_PHASE
    rng = np.random.default_rng(400)
    f = np.stack([np.full((B, T), 7999.0), rng.uniform(7000.0, 7990.0, (B, T))], -1)
    return dict(shape=LARGE_PHASE, track="large", normalize=True, f=f.astype(np.float32),
                c=rng.uniform(0.5, 2.0, (B, T, K)).astype(np.float32), a=rng.uniform(0.5, 1.5, (B, T, 1)).astype(np.float32))


def invalid_entries(case, rng):
    """NaN, +-inf and negative frequencies scattered over a copy of the case (about one entry in six)"""
    f = case["f"].copy()
    bad = rng.random(f.shape) < 1.0 / 6.0
    f[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, -1.0, -440.0], np.float32), int(bad.sum()))
    return dict(case, f=f), bad


def backward_cases():
    """The first five shapes.  With K = 1 a normalised weight is 1 whatever c is, so grad_c is zero by cancellation and no bound
    is small against it: that shape runs without the normalisation.  -> list of (case, grad_y, invalid entries or None)"""
    out = []
    for i, shape in enumerate(SHAPES[:5]):
        B, T, K, hop = shape
        rng = np.random.default_rng(500 + i)
        norms = (False,) if K == 1 else (True, False)
        for normalize in norms:
            for j, track in enumerate(("random", "octaves", "nyquist")):
                case = make_case(shape, track, 600 + 10 * i + j, normalize)
                out.append((case, rng.standard_normal((B, T * hop)), None))
            case, bad = invalid_entries(make_case(shape, "nyquist", 650 + i, normalize), rng)
            out.append((case, rng.standard_normal((B, T * hop)), bad))
    return out
