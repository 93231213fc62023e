"""The averaged (EMA) weights restated in numpy: the host weight schedule and one update.
Nothing here calls the library; tests compare the library's bits with these."""
import numpy as np


def weight(decay, t):
    """w_t = (float)(1 - min(decay, (1 + t) / (10 + t))), t = updates made so far (0-based); the arithmetic is
    double until the one rounding to float32."""
    d = min(float(decay), (1.0 + float(t)) / (10.0 + float(t)))
    return np.float32(1.0 - d)


def update(e, p, w):
    """e + w * (p - e) on float32 arrays: numpy rounds each of the three operations once and never fuses."""
    e = np.asarray(e, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return e + np.float32(w) * (p - e)


def update64(e, p, w):
    """The same recurrence in float64 (the same w_t, a float32 value by definition): the yardstick of the three
    float32 roundings' error."""
    return np.asarray(e, dtype=np.float64) + float(w) * (np.asarray(p, dtype=np.float64) - e)
