"""bagged_forest_predict_kernel against sklearn's own fp64 results, bit for
bit: every model of bagged_fixtures at B = 1, R - 1, R + 1, 2R + 3 under three
(prefix, chunk) settings, the binding's preconditions, and the random-forest
app."""

import numpy as np
import pytest
import torch
from bagged_fixtures import MODELS, fitted, probe_rows, sklearn_means

from unionml_amd.ops import forest as F

pytestmark = pytest.mark.gpu
POISON_PROB, POISON_LABEL = -7.25, -5


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    return hip_ext(required=True)


@pytest.fixture(scope="module")
def cases():
    """name -> (estimator, device forest, probe rows, the same on the device,
    sklearn's means of those rows), each built once."""
    out = {}

    def get(name):
        if name not in out:
            est = fitted(name)
            forest = F.from_sklearn(est, device="cuda")
            X = probe_rows(name, forest, 2 * forest.rows_per_wg + 3)
            out[name] = (est, forest, X, torch.from_numpy(X).cuda(), sklearn_means(est, X))
        return out[name]

    return get


def launch(ext, forest, X, B, prefix_nodes, trees_per_chunk, spare=3):
    probs = torch.full((B + spare, forest.n_scores), POISON_PROB, dtype=torch.float64,
                       device="cuda")
    labels = torch.full((B + spare,), POISON_LABEL, dtype=torch.int32, device="cuda")
    ext.bagged_forest_predict(X[:B], forest._nodes, forest._first, forest._values,
                              forest.max_tree_nodes, probs, labels, prefix_nodes,
                              trees_per_chunk)
    return probs, labels


@pytest.mark.parametrize("prefix_nodes,trees_per_chunk", [(-1, 0), (0, 1), (3, 5)])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_kernel_equals_sklearn_bit_for_bit(ext, cases, name, prefix_nodes, trees_per_chunk):
    est, forest, X, Xd, want = cases(name)
    R = forest.rows_per_wg
    assert R == ext.bagged_rows_per_wg(forest.n_features, forest.n_scores)
    for B in (1, R - 1, R + 1, 2 * R + 3):
        probs, labels = launch(ext, forest, Xd, B, prefix_nodes, trees_per_chunk)
        ref = torch.from_numpy(want[:B]).cuda()
        assert torch.equal(probs[:B], ref), (name, B)
        assert torch.equal(labels[:B], ref.argmax(dim=1).int()), (name, B)
        assert bool((probs[B:] == POISON_PROB).all()) and bool((labels[B:] == POISON_LABEL).all())
    finite = ~np.isinf(X).any(axis=1)   # sklearn's public methods refuse +-inf
    if hasattr(est, "classes_"):
        assert torch.equal(forest.predict_proba(Xd, prefix_nodes, trees_per_chunk).cpu(),
                           torch.from_numpy(want))
        assert np.array_equal(forest.predict(Xd, prefix_nodes, trees_per_chunk)[finite],
                              est.predict(X[finite]))
    else:
        assert np.array_equal(forest.predict(Xd, prefix_nodes, trees_per_chunk).cpu().numpy(),
                              est.predict(X))


def test_replays_of_a_captured_launch_equal_the_eager_result(ext, cases):
    _, forest, _, Xd, _ = cases("rf_digits")
    B = forest.rows_per_wg + 1
    probs, labels = launch(ext, forest, Xd, B, -1, 0)   # the capture is not the first launch
    gp, gl = torch.empty_like(probs), torch.empty_like(labels)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # records, does not run
        ext.bagged_forest_predict(Xd[:B], forest._nodes, forest._first, forest._values,
                                  forest.max_tree_nodes, gp, gl)
    for _ in range(3):
        gp.fill_(POISON_PROB)
        gl.fill_(POISON_LABEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gp, probs) and torch.equal(gl, labels)


def test_constants_match_the_header(ext):
    assert (ext.BAGGED_MAX_CLASSES, ext.BAGGED_MAX_FEATURES, ext.BAGGED_MAX_TREE_NODES,
            ext.BAGGED_MAX_ROWS, ext.BAGGED_META_DIST_SHIFT, ext.BAGGED_META_MISSING_LEFT,
            ext.BAGGED_TILE_BYTES) == (
        F.MAX_CLASSES, F.MAX_FEATURES, F.BAGGED_MAX_TREE_NODES, F.BAGGED_MAX_ROWS,
        F.BAGGED_META_DIST_SHIFT, F.BAGGED_META_MISSING_LEFT, F.BAGGED_TILE_BYTES)
    for f, k in ((64, 10), (64, 32), (5, 2), (300, 3), (1, 1), (2048, 1), (2049, 1), (4, 33)):
        assert ext.bagged_rows_per_wg(f, k) == F.bagged_rows_per_wg(f, k)
    for rows, trees, cap in ((1, 100, 0), (1, 1000, 0), (3, 7, 0), (128, 100, 0), (65, 100, 5)):
        assert ext.bagged_trees_per_chunk(rows, trees, cap) == F.bagged_trees_per_chunk(
            rows, trees, cap)


@pytest.mark.parametrize("broken", ["dtype", "k_width", "short_labels", "strided_x", "aliased"])
def test_binding_preconditions(ext, cases, broken):
    _, forest, _, Xd, _ = cases("single_tree")
    B, K = 40, forest.n_scores
    args = dict(X=Xd[:B].clone(),
                probs=torch.full((B, K), POISON_PROB, dtype=torch.float64, device="cuda"),
                labels=torch.full((B,), POISON_LABEL, dtype=torch.int32, device="cuda"))
    if broken == "dtype":
        args["X"] = args["X"].double()
    elif broken == "k_width":
        args["probs"] = torch.full((B, K + 1), POISON_PROB, dtype=torch.float64, device="cuda")
    elif broken == "short_labels":
        args["labels"] = args["labels"][: B - 1]
    elif broken == "strided_x":
        args["X"] = torch.cat([args["X"], args["X"]], dim=1)[:, ::2]
    elif broken == "aliased":
        args["labels"] = args["X"].view(torch.int32).view(-1)[:B]
    kept = {k: v.clone().contiguous() for k, v in args.items()}
    with pytest.raises(RuntimeError):
        ext.bagged_forest_predict(args["X"], forest._nodes, forest._first, forest._values,
                                  forest.max_tree_nodes, args["probs"], args["labels"])
    torch.cuda.synchronize()
    assert all(torch.equal(v.contiguous().view(torch.uint8), kept[k].view(torch.uint8))
               for k, v in args.items())


def test_random_forest_app_predicts_on_the_device():
    from unionml_amd.models import rforest

    rforest.model.artifact = None
    clf, _ = rforest.model.train(trainer_kwargs={"n_estimators": 20}, n=400)
    frame = rforest.reader(n=400)[rforest.FEATURES]
    got = rforest.predictor(clf, frame)
    assert rforest.device_forest(clf) is rforest.device_forest(clf)
    assert got == [int(c) for c in clf.predict(frame)]
