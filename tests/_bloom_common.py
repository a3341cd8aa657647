"""What the bloom tests share: the images, the cases, the twin's measured bounds and the error measure."""
import numpy as np

F32 = np.float32
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 31), (64, 64), (255, 257)]           # (w, h)
LEVELS = [1, 2, 6, 12]
THRESHOLDS = [dict(threshold=0.0), dict(threshold=1.0, knee=0.0), dict(threshold=1.0, knee=0.5), dict(threshold=1.0, knee=1.0)]
SCATTERS = [0.0, 0.7, 1.0]

# max |got - want| / max(|want|, 1e-3) of the host twin against the binary64 restatement over every case of test_bloom_cpu.py's sweep,
# measured on the twin (never on the device); the bounds are 4 x the measurements (the convention of DESIGN.md 3.1)
MEASURED_PLAIN, MEASURED_KARIS = 5.33e-7, 1.02e-6
BOUND_PLAIN, BOUND_KARIS = 4 * MEASURED_PLAIN, 4 * MEASURED_KARIS


def log_uniform(rng, shape, lo=-12.0, hi=6.0):
    return np.exp2(rng.uniform(lo, hi, shape)).astype(F32)


def image(w, h, seed=0):
    return log_uniform(np.random.default_rng(1000 * w + h + seed), (h, w, 3))


def salted(w=37, h=53, clamp_max=65504.0):
    """a random image with NaN, +-inf, -1, +-0, a subnormal, clamp_max and its successor in it; returns it and the same image with
    every channel that must stay what it is replaced by what the prefilter makes of it (0, or clamp_max for +inf)"""
    img = image(w, h, seed=7)
    salt = [np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-41, clamp_max, float(np.nextafter(F32(clamp_max), F32(np.inf)))]
    rng = np.random.default_rng(3)
    flat = img.reshape(-1)
    at = rng.choice(flat.size, 4 * len(salt), replace=False)
    for n, i in enumerate(at):
        flat[i] = F32(salt[n % len(salt)])
    img[0, 0] = (np.nan, np.inf, -1.0)                                             # a whole pixel, in a corner
    img[h - 1, w - 1] = (-np.inf, -0.0, np.nan)
    clean = img.copy()
    with np.errstate(invalid="ignore"):
        clean[~(img > 0)] = 0.0
    clean[np.isposinf(img)] = F32(clamp_max)
    return img, clean


def err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1e-3))) if want.size else 0.0


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)
