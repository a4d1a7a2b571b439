"""Forest fixture (tests/golden/forest.npz).

Fits three scikit-learn ensembles on about 2,000 seeded rows of 39 features
and records, per ensemble, the node tables as vad_amd.forest.ForestClassifier
lays them out (the trees one after another, child indices absolute, bagged
features mapped back to the full row), ``estimators_features_`` where there
are any, and sklearn's own ``predict_proba`` and ``predict`` (n_jobs=1) on a
few hundred held-out rows, some with NaN features.  The fixture pins the
averaging and the traversal, not a model.  Only arrays are stored (no pickle).

    python tests/golden/gen_forest.py
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.ensemble import BaggingClassifier, RandomForestClassifier
from sklearn.tree import DecisionTreeClassifier

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

N_TRAIN, N_TEST, F = 2000, 300, 39


def rows(n, K, seed):
    """Class centres in the first 12 columns, noise elsewhere, 10% of the labels flipped."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, K, n)
    centres = np.random.default_rng(1234 + K).normal(0.0, 1.0, (K, F)) * (np.arange(F) < 12)
    x = (centres[y] + rng.normal(0.0, 1.5, (n, F))).astype(np.float32)
    flip = rng.random(n) < 0.10
    y[flip] = rng.integers(0, K, int(flip.sum()))
    return x, y


def estimators():
    """name -> (unfitted estimator, n_classes, class values)"""
    return {
        "rf": (RandomForestClassifier(n_estimators=5, max_depth=6, n_jobs=1, random_state=0), 2, np.array([0, 1])),
        "bag": (BaggingClassifier(DecisionTreeClassifier(max_depth=5), n_estimators=4, max_samples=0.6,
                                  max_features=0.5, bootstrap=False, random_state=0), 2, np.array([0, 1])),
        "rf3": (RandomForestClassifier(n_estimators=6, max_depth=7, n_jobs=1, random_state=1), 3,
                np.array([2, 5, 9])),
    }


def fitted(name):
    est, K, values = estimators()[name]
    x, y = rows(N_TRAIN, K, seed=11 + K)
    return est.fit(x, values[y])


def test_rows(K):
    xt, _ = rows(N_TEST, K, seed=99 + K)
    xt[::37, 0] = np.nan  # NaN rows: missing_go_to_left
    xt[5::41, 7] = np.nan
    return xt


def main():
    from vad_amd.forest import ForestClassifier
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (_, K, _) in estimators().items():
        clf = fitted(name)
        f = ForestClassifier.from_sklearn(clf)
        xt = test_rows(K)
        for k in ("feature", "threshold", "left", "right", "leaf", "nan_left", "roots", "proba"):
            out[f"{name}_{k}"] = getattr(f, k)
        out[f"{name}_classes"] = f.classes_
        out[f"{name}_x_test"] = xt
        out[f"{name}_predict_proba"] = clf.predict_proba(xt)
        out[f"{name}_predict"] = clf.predict(xt)
        if hasattr(clf, "estimators_features_"):
            out[f"{name}_estimators_features"] = np.stack(clf.estimators_features_)
        print(name, "trees", f.n_trees, "nodes", len(f.feature), "test rows", len(xt))
    np.savez_compressed(os.path.join(HERE, "forest.npz"), **out)


if __name__ == "__main__":
    main()
