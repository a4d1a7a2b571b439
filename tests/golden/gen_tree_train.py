"""Generates tests/golden/tree_train.npz: rows, labels and the arrays of
sklearn DecisionTreeClassifier trees (criterion gini, best splitter) fitted to
them, for the node-by-node check of the training rule
(tests/test_tree_train_cpu.py).  Uses sklearn only; written with 1.7.2.

    python tests/golden/gen_tree_train.py
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.tree import DecisionTreeClassifier

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tree_train_reference as R  # noqa: E402

# name: (rows, features, classes, seed, max_depth, min_samples_split, min_samples_leaf)
CONFIGS = {
    "a39": (1200, 39, 3, 101, 25, 22, 20),
    "b13": (2500, 13, 2, 102, 6, 22, 20),
    "c7q": (3000, 7, 3, 103, 25, 10, 5),
    "d5": (3000, 5, 2, 104, 25, 2, 1),
}
STATES = (0, 1, 2, 3)


def rows_of(name):
    n, F, K, seed = CONFIGS[name][:4]
    x, y = R.synth(n, F, K, seed)
    if name == "c7q":  # every informative column quantised: many equal values and tied scores
        x[:, :3] = np.round(x[:, :3] * 2) / 2
    return x, y


def main():
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (n, F, K, seed, md, mss, msl) in CONFIGS.items():
        x, y = rows_of(name)
        out[f"{name}_x"], out[f"{name}_y"] = x, y
        out[f"{name}_params"] = np.array([K, md, mss, msl], np.int64)
        for rs in STATES:
            t = DecisionTreeClassifier(max_depth=md, min_samples_split=mss, min_samples_leaf=msl,
                                       random_state=rs).fit(x, y).tree_
            pre = f"{name}_rs{rs}_"
            out[pre + "left"] = np.asarray(t.children_left, np.int32)
            out[pre + "right"] = np.asarray(t.children_right, np.int32)
            out[pre + "feature"] = np.asarray(t.feature, np.int32)
            out[pre + "threshold"] = np.asarray(t.threshold, np.float64)
            out[pre + "n_node_samples"] = np.asarray(t.n_node_samples, np.int32)
            out[pre + "missing_go_to_left"] = np.asarray(t.missing_go_to_left, np.uint8)
    path = os.path.join(HERE, "tree_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
