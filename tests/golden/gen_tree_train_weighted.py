"""Generates tests/golden/tree_train_weighted.npz: rows, labels, integer row
weights and the arrays of sklearn DecisionTreeClassifier trees fitted with
``sample_weight=`` those weights, for the node-by-node check of the weighted
training rule (tests/test_tree_train_weighted_cpu.py).  Uses sklearn only;
written with 1.7.2.

Per configuration three weight kinds: bootstrap counts ("boot"), one integer
per class ("class") and their product ("both").  The generator runs the
node-wise check itself and fails if any node of any tree fails it, so the
committed fixture is one the rule passes in full.  (On other rows sklearn's
choice can miss the rule's maximum by one rounding where two candidates tie in
exact arithmetic: DESIGN.md section 4, "Integer row weights".)

    python tests/golden/gen_tree_train_weighted.py
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.tree import DecisionTreeClassifier

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tree_train_weighted_reference as W  # noqa: E402

# name: (rows, features, classes, seed, max_depth, min_samples_split, min_samples_leaf)
CONFIGS = {
    "w13": (2500, 13, 2, 202, 6, 22, 20),
    "w7q": (3000, 7, 3, 203, 25, 10, 5),
    "w5": (2000, 5, 2, 204, 25, 2, 1),
    "w9": (1500, 9, 3, 205, 25, 40, 20),
}
KINDS = ("boot", "class", "both")
STATES = (0, 1, 2, 3)


def rows_of(name):
    n, F, K, seed = CONFIGS[name][:4]
    x, y = W.synth(n, F, K, seed)
    if name == "w7q":  # every informative column quantised: many equal values and tied scores
        x[:, :3] = np.round(x[:, :3] * 2) / 2
    return x, y


def main():
    out = {"sklearn_version": np.array(sklearn.__version__)}
    nodes = splits = ties = 0
    for name, (n, F, K, seed, md, mss, msl) in CONFIGS.items():
        x, y = rows_of(name)
        out[f"{name}_x"], out[f"{name}_y"] = x, y
        out[f"{name}_params"] = np.array([K, md, mss, msl], np.int64)
        for kind in KINDS:
            w = W.weights_of(kind, y, K, seed)
            assert w.max() <= 255 and w.sum() <= W.MAX_TOTAL
            out[f"{name}_{kind}_w"] = w.astype(np.uint8)
            for rs in STATES:
                t = DecisionTreeClassifier(max_depth=md, min_samples_split=mss, min_samples_leaf=msl,
                                           random_state=rs).fit(x, y, sample_weight=w.astype(np.float64)).tree_
                pre = f"{name}_{kind}_rs{rs}_"
                out[pre + "left"] = np.asarray(t.children_left, np.int32)
                out[pre + "right"] = np.asarray(t.children_right, np.int32)
                out[pre + "feature"] = np.asarray(t.feature, np.int32)
                out[pre + "threshold"] = np.asarray(t.threshold, np.float64)
                out[pre + "n_node_samples"] = np.asarray(t.n_node_samples, np.int32)
                out[pre + "missing_go_to_left"] = np.asarray(t.missing_go_to_left, np.uint8)
                out[pre + "weighted_n_node_samples"] = np.asarray(t.weighted_n_node_samples, np.float64)
                out[pre + "value"] = np.asarray(t.value[:, 0, :], np.float64)
                a, b, c = W.check_tree_nodewise(x, y, w, K, md, mss, msl, out[pre + "left"], out[pre + "right"],
                                                out[pre + "feature"], out[pre + "threshold"],
                                                out[pre + "n_node_samples"], out[pre + "missing_go_to_left"],
                                                out[pre + "weighted_n_node_samples"], out[pre + "value"])
                nodes, splits, ties = nodes + a, splits + b, ties + c
    print(f"{nodes} nodes, {splits} splits, {ties} with a score tie between features: every node passes")
    path = os.path.join(HERE, "tree_train_weighted.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
