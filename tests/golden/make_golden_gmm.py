"""Writes tests/golden/gmm.npz: scikit-learn 1.7's own values for the cases of tests/gmm_cases.py (needs scikit-learn
only; run from the repository root: ``python tests/golden/make_golden_gmm.py``).

Per step case: the parameters, sklearn's ``_estimate_log_prob_resp`` there and sklearn's ``_m_step`` at the
restatement's responsibilities.  Per fit case: sklearn's fitted attributes from the same start (explicit ``*_init``
arrays; ``init_params='random_from_data'`` with the same seed; for the k-means start the restatement's start handed over
as ``weights_init`` / ``means_init`` / ``precisions_init``).  sklearn always gets the float64 copy of the rows.

Beside every quantity ``q`` the file stores ``floor_q``: the larger of |sklearn - restatement| and |sklearn - sklearn on
rows perturbed by 1e-15 relative|, relative to max |sklearn|.  That is the reference-side noise the tests scale their
bounds with.

Per limit case (``GC.LIMIT_CASES``; the covariances of 64 components in 128 dimensions are 8 MB, so neither parameters
nor covariances are stored): sklearn's ``log_prob_norm`` at the case's explicit parameters and ``GC.limit_reduced`` of
sklearn's ``_m_step`` at ``GC.limit_resp``, each with its floor.  The float64 copy of the corner shares the float32
copy's entries."""
import os
import sys
import warnings

import numpy as np
from sklearn.mixture import GaussianMixture

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gmm_cases as GC  # noqa: E402

warnings.filterwarnings("ignore")
STEP_GOLDEN = ["n33_d5_k3", "n17_d16_k17", "n2049_d33_k2", "duplicates", "offset", "small_weight", "empty"]
PERTURBATION = 1e-15


def step_inputs(name, cov_type):
    if name in GC.STEP_CASES:
        return GC.step_case(name, cov_type)
    if name == "empty":
        return GC.empty_case(cov_type)
    if name == "small_weight":
        return GC.small_weight_case(cov_type)
    return GC.special_case(name, cov_type)


def perturbed(X, salt):
    rng = np.random.RandomState(salt)
    return np.asarray(X, dtype=np.float64) * (1.0 + PERTURBATION * rng.standard_normal(X.shape))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    scale = np.abs(a[ok]).max() if ok.any() else 1.0
    return float(np.abs(a[ok] - b[ok]).max() / max(scale, np.finfo(float).tiny)) if ok.any() else 0.0


def sk_e_step(X, weights, means, pchol, cov_type):
    gm = GaussianMixture(len(weights), covariance_type=cov_type)
    gm.weights_, gm.means_, gm.precisions_cholesky_ = weights, means, pchol
    return gm._estimate_log_prob_resp(np.asarray(X, dtype=np.float64))


def sk_m_step(X, resp, cov_type):
    gm = GaussianMixture(resp.shape[1], covariance_type=cov_type, reg_covar=1e-6)
    with np.errstate(divide="ignore"):
        gm._m_step(np.asarray(X, dtype=np.float64), np.log(resp))
    return gm.weights_, gm.means_, gm.covariances_, gm.precisions_cholesky_


def sk_fit(X, k, cov_type, init, params, tol, max_iter):
    kw = dict(covariance_type=cov_type, tol=tol, max_iter=max_iter, reg_covar=1e-6)
    if init == "explicit":
        w, mu, prec = GC.explicit_init(X, k, cov_type)
        kw.update(weights_init=w, means_init=mu, precisions_init=prec)
    elif init == "random_from_data":
        kw.update(init_params="random_from_data", random_state=42)
    else:
        w, mu, _, pchol = params
        prec = np.array([p @ p.T for p in pchol]) if cov_type == "full" else pchol ** 2
        kw.update(weights_init=w, means_init=mu, precisions_init=prec)
    gm = GaussianMixture(k, **kw).fit(X)
    return dict(weights=gm.weights_, means=gm.means_, covariances=gm.covariances_,
                precisions_cholesky=gm.precisions_cholesky_, lower_bound=np.float64(gm.lower_bound_),
                n_iter=np.int64(gm.n_iter_), converged=np.bool_(gm.converged_))


def main():
    out = {}
    for name in STEP_GOLDEN:
        for cov_type in GC.COV_TYPES:
            X, weights, means, cov, pchol, lpn, log_resp, resp = step_inputs(name, cov_type)
            key = "%s_%s_" % (name, cov_type)
            out[key + "weights"], out[key + "means"], out[key + "pchol"] = weights, means, pchol
            sk = sk_e_step(X, weights, means, pchol, cov_type)
            sp = sk_e_step(perturbed(X, 1), weights, means, pchol, cov_type)
            seen = resp >= 1e-300
            floors = []
            for q, got, a, b in (("lpn", lpn, sk[0], sp[0]),
                                 ("log_resp", np.where(seen, log_resp, 0.0), np.where(seen, sk[1], 0.0),
                                  np.where(seen, sp[1], 0.0))):
                out[key + q] = a
                out[key + "floor_" + q] = np.float64(max(rel(a, got), rel(a, b)))
                floors.append(out[key + "floor_" + q])
            skm = sk_m_step(X, resp, cov_type)
            spm = sk_m_step(perturbed(X, 2), resp, cov_type)
            mine = GC.m_step(X, resp, 1e-6, cov_type)
            for q, got, a, b in zip(("m_weights", "m_means", "m_cov", "m_pchol"), mine, skm, spm):
                out[key + q] = a
                out[key + "floor_" + q] = np.float64(max(rel(a, got), rel(a, b)))
                floors.append(out[key + "floor_" + q])
            print("%-14s %-4s floors: %s" % (name, cov_type, " ".join("%.1e" % f for f in floors)))
    before = sum(np.asarray(v).nbytes for v in out.values())
    for name in GC.LIMIT_CASES:
        for cov_type in GC.COV_TYPES:
            key = GC.limit_key(name, cov_type)
            if key + "lpn" in out:
                continue
            X, weights, means, cov, pchol, lpn, _, _ = GC.limit_case(name, cov_type)
            sk = sk_e_step(X, weights, means, pchol, cov_type)[0]
            sp = sk_e_step(perturbed(X, 1), weights, means, pchol, cov_type)[0]
            out[key + "lpn"] = sk
            out[key + "floor_lpn"] = np.float64(max(rel(sk, lpn), rel(sk, sp)))
            floors = [out[key + "floor_lpn"]]
            resp = GC.limit_resp(name)
            skm = GC.limit_reduced(*sk_m_step(X, resp, cov_type), cov_type)
            spm = GC.limit_reduced(*sk_m_step(perturbed(X, 2), resp, cov_type), cov_type)
            mine = GC.limit_reduced(*GC.m_step(X, resp, 1e-6, cov_type), cov_type)
            for q, got, a, b in zip(GC.LIMIT_QUANTITIES, mine, skm, spm):
                out[key + q] = a
                out[key + "floor_" + q] = np.float64(max(rel(a, got), rel(a, b)))
                floors.append(out[key + "floor_" + q])
            print("%-14s %-4s floors: %s" % (name, cov_type, " ".join("%.1e" % f for f in floors)))
    print("limit cases: %d bytes of arrays" % (sum(np.asarray(v).nbytes for v in out.values()) - before))
    for case in GC.FIT_CASES:
        name, cov_type, init, run = case
        tol, max_iter = {r[0]: r[1:] for r in GC.FIT_RUNS}[run]
        X, k, params, _ = GC.fit_start(name, cov_type, init)
        mine = GC.fit_case(*case)
        X64 = np.asarray(X, dtype=np.float64)
        sk = sk_fit(X64, k, cov_type, init, params, tol, max_iter)
        sp = sk_fit(perturbed(X, 3), k, cov_type, init, params, tol, max_iter)
        key = GC.fit_id(case) + "_"
        floors = []
        for q in GC.FIT_QUANTITIES:
            out[key + q] = sk[q]
            out[key + "floor_" + q] = np.float64(max(rel(sk[q], mine[q]), rel(sk[q], sp[q])))
            floors.append(out[key + "floor_" + q])
        out[key + "n_iter"], out[key + "converged"] = sk["n_iter"], sk["converged"]
        print("%-44s n_iter %3d (restatement %3d) converged %d floors: %s"
              % (GC.fit_id(case), sk["n_iter"], mine["n_iter"], sk["converged"], " ".join("%.1e" % f for f in floors)))
    path = os.path.join(HERE, "gmm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
