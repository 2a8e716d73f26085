"""``evaluation/metrics.py`` — safety statistics of per-realisation clearances, host and device.

Reference: ``collision_rate`` (:6-16), ``expectation_of_shortfall`` (:18-32), ``safety_metrics``
(:34-65): same names, same keys, quantiles by ``np.percentile``'s linear interpolation.

Every function takes a NumPy array (the reference's own NumPy calls, value for value) or a float64
device tensor.  A device tensor is reduced on the device by torch ops — one sort serves the five
quantiles, the minimum and the maximum; ``torch.quantile`` is not used, it refuses more than 16 M
elements — and the results come back as Python floats in one copy.  Non-finite clearances give what
the NumPy calls give: a NaN among them makes the minimum and every quantile NaN (the sort puts NaN
last, so the sorted order alone would read past it), an all-+inf sample has the median +inf.
"""
from __future__ import annotations

import numpy as np
import torch

_QUANTILES = (("q10", 10.0), ("q25", 25.0), ("median", 50.0), ("q75", 75.0), ("q90", 90.0))


def _is_device(distances) -> bool:
    if not isinstance(distances, torch.Tensor):
        return False
    if distances.dtype != torch.float64:
        raise ValueError("a tensor of clearances must be float64")
    return True


def _shortfall_t(d, threshold):
    """Mean of (d - threshold) over d < threshold, 0 where there is none: a 0-d tensor."""
    below = d < threshold
    n = below.sum()
    total = torch.where(below, d - threshold, torch.zeros_like(d)).sum()
    return torch.where(n > 0, total / n.clamp(min=1).to(d.dtype), torch.zeros_like(total))


def collision_rate(distances):
    """Share of the runs whose minimum clearance is negative (:6-16)."""
    if _is_device(distances):
        return float((distances.reshape(-1) < 0).to(torch.float64).mean())
    return np.mean(np.asarray(distances) < 0)


def expectation_of_shortfall(distances, threshold=0):
    """Mean clearance below ``threshold``, relative to it; 0.0 if no run is below (:18-32)."""
    if _is_device(distances):
        return float(_shortfall_t(distances.reshape(-1), threshold))
    distances = np.asarray(distances)
    shortfalls = distances[distances < threshold]
    if len(shortfalls) == 0:
        return 0.0
    return np.mean(shortfalls - threshold)


def safety_metrics(distances, threshold=0):
    """mean, min, max, std, collision_rate, expected_shortfall, q10, q25, median, q75, q90 (:34-65)."""
    if _is_device(distances):
        return _safety_metrics_device(distances.reshape(-1), threshold)
    distances = np.asarray(distances)
    metrics = {"mean": np.mean(distances), "min": np.min(distances), "max": np.max(distances),
               "std": np.std(distances), "collision_rate": collision_rate(distances),
               "expected_shortfall": expectation_of_shortfall(distances, threshold)}
    for key, q in _QUANTILES:
        metrics[key] = np.median(distances) if key == "median" else np.percentile(distances, q)
    return metrics


def _safety_metrics_device(d, threshold):
    n = d.numel()
    if n == 0:
        raise ValueError("safety_metrics needs at least one clearance")
    s, _ = torch.sort(d)
    # the sort puts NaN last: s[-1] is NaN exactly when a clearance is.  NumPy's minimum and
    # quantiles of such a sample are NaN; the sorted order alone would skip the NaN.
    undefined = torch.isnan(s[-1])
    nan = torch.full_like(s[-1], float("nan"))
    vals = [d.mean(), torch.where(undefined, nan, s[0]), s[-1], d.std(unbiased=False),
            (d < 0).to(torch.float64).mean(), _shortfall_t(d, threshold)]
    for key, q in _QUANTILES:
        # np.percentile, method "linear": virtual index q/100 (n - 1), interpolated between its
        # neighbours in the sorted order
        pos = q / 100.0 * (n - 1)
        lo = min(int(np.floor(pos)), n - 1)
        hi = min(lo + 1, n - 1)
        v = torch.lerp(s[lo], s[hi], pos - lo)
        if key == "median":
            # np.median is the mean of the middle element(s), which infinite neighbours leave
            # defined where the interpolation's difference does not (+inf: the empty obstacle grid)
            a, b = s[lo], (s[lo] if pos == lo else s[hi])
            v = torch.where(torch.isfinite(v), v, (a + b) / 2)
        vals.append(torch.where(undefined, nan, v))
    host = torch.stack(vals).tolist()
    keys = ["mean", "min", "max", "std", "collision_rate", "expected_shortfall"] + [k for k, _ in _QUANTILES]
    return dict(zip(keys, host))
