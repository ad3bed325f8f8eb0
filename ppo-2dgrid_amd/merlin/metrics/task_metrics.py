"""Distances between two sets of per-task features (rewards, states, embeddings): the definitions of the
reference's src/metrics/task_metrics.py, which distribution_over_tasks.py reports on the two policies' rewards.

Each set is summarised as a diagonal Gaussian (per-dimension mean, population std + 1e-8):
  KL(P || Q)   sum_d  log(s_q / s_p) + (s_p^2 + (m_p - m_q)^2) / (2 s_q^2) - 1/2
  JS(P, Q)     (KL(P || M) + KL(Q || M)) / 2 with M the Gaussian of the averaged means and averaged stds
               (not the moment-matched mixture)
  Wasserstein  per dimension, mean |sorted(u)[k] - sorted(v)[k]| over the first min(len) order statistics
               (the longer sample is truncated after sorting, not resampled), averaged over dimensions.
numpy only, float64 throughout.
"""
from __future__ import annotations

import itertools

import numpy as np

STD_FLOOR = 1e-8


def _as_2d(x):
    x = np.asarray(x)
    return x.reshape(-1, 1) if x.ndim == 1 else x


def compute_mean_std(features):
    """(mean [D], std [D] + 1e-8) of samples [N, D] (or [N])."""
    x = _as_2d(features)
    return x.mean(axis=0), x.std(axis=0) + STD_FLOOR


def kl_diag_gaussians(mean_p, std_p, mean_q, std_q) -> float:
    log_ratio = np.log(std_q / std_p)
    quad = (std_p ** 2 + (mean_p - mean_q) ** 2) / (2.0 * std_q ** 2)
    return float(np.sum(log_ratio + quad - 0.5))


def js_diag_gaussians(mean_p, std_p, mean_q, std_q) -> float:
    mean_m, std_m = 0.5 * (mean_p + mean_q), 0.5 * (std_p + std_q)
    return float(0.5 * (kl_diag_gaussians(mean_p, std_p, mean_m, std_m)
                        + kl_diag_gaussians(mean_q, std_q, mean_m, std_m)))


def wasserstein_1d(u, v) -> float:
    u, v = np.sort(np.asarray(u).ravel()), np.sort(np.asarray(v).ravel())
    n = min(u.size, v.size)
    if n == 0:
        return 0.0
    return float(np.mean(np.abs(u[:n] - v[:n])))


def wasserstein_mean(features_p, features_q) -> float:
    x, y = _as_2d(features_p), _as_2d(features_q)
    return float(np.mean([wasserstein_1d(x[:, d], y[:, d]) for d in range(x.shape[1])]))


def compare_two_feature_sets(feats_a, feats_b) -> dict:
    """{"mean_norm_diff", "kl_ab", "kl_ba", "js_div", "wasserstein"} of samples [N_a, D] and [N_b, D]."""
    mean_a, std_a = compute_mean_std(feats_a)
    mean_b, std_b = compute_mean_std(feats_b)
    return {
        "mean_norm_diff": float(np.linalg.norm(mean_a - mean_b)),
        "kl_ab": kl_diag_gaussians(mean_a, std_a, mean_b, std_b),
        "kl_ba": kl_diag_gaussians(mean_b, std_b, mean_a, std_a),
        "js_div": js_diag_gaussians(mean_a, std_a, mean_b, std_b),
        "wasserstein": wasserstein_mean(feats_a, feats_b),
    }


def compare_task_feature_dict(feature_dict) -> dict:
    """{(task_i, task_j): compare_two_feature_sets} for every unordered pair, in the dict's order."""
    return {(a, b): compare_two_feature_sets(feature_dict[a], feature_dict[b])
            for a, b in itertools.combinations(list(feature_dict), 2)}
