"""The split walk (forest_split_walk_kernel + forest_split_sum_kernel) against
sklearn's own fp64 scores, bit for bit: every model of forest_fixtures and a
regressor of 5,999-node trees under three (prefix, slice) caps, the forced
paths against each other, the binding's preconditions and a graph replay."""

import numpy as np
import pytest
import torch
from forest_fixtures import MODELS, fitted, probe_rows, raw_argmax_labels, sklearn_scores
from forest_split_fixtures import grown

from unionml_amd.ops import forest as F

pytestmark = pytest.mark.gpu
CAPS = [(-1, 0), (0, 1), (3, 5)]     # (prefix_nodes, trees_per_slice)


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    return hip_ext(required=True)


@pytest.fixture(scope="module")
def cases():
    """name -> (estimator, device forest, probe rows on the device, sklearn's
    scores of those rows), each built once."""
    out = {}

    def get(name):
        if name not in out:
            est = fitted(name)
            forest = F.ForestPredictor.from_sklearn(est, device="cuda")
            X = probe_rows(forest, 2 * forest.split_rows_per_wg + 17)
            out[name] = (est, forest, torch.from_numpy(X).cuda(), sklearn_scores(est, X))
        return out[name]

    return get


@pytest.mark.parametrize("prefix_nodes,trees_per_slice", CAPS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_split_walk_equals_sklearn_bit_for_bit(ext, cases, name, prefix_nodes, trees_per_slice):
    est, forest, X, want = cases(name)
    assert forest.split_rows_per_wg == ext.forest_split_rows_per_wg(forest.n_features)
    # two full row tiles and a short one; the lone row; RP > rows
    for B in (len(X), 1, 3):
        got = forest.decision_function(X[:B], walk="split", prefix_nodes=prefix_nodes,
                                       trees_per_slice=trees_per_slice)
        assert torch.equal(got, torch.from_numpy(want[:B]).cuda()), (name, B)
        if hasattr(est, "classes_"):
            labels = forest.predict(X[:B], walk="split", prefix_nodes=prefix_nodes,
                                    trees_per_slice=trees_per_slice)
            assert np.array_equal(labels, raw_argmax_labels(est, want[:B])), (name, B)


@pytest.mark.parametrize("prefix_nodes,trees_per_slice", CAPS[:2])
def test_grown_regressor(prefix_nodes, trees_per_slice):
    est, X, want = grown()
    assert max(len(t.nodes) for it in est._predictors for t in it) > F.CHUNK_NODES
    forest = F.ForestPredictor.from_sklearn(est, device="cuda")
    assert forest._nodes is None and forest.walk_for(len(X)) == "split"
    got = forest.predict(torch.from_numpy(X).cuda(), prefix_nodes=prefix_nodes,
                         trees_per_slice=trees_per_slice)
    assert torch.equal(got, torch.from_numpy(want).cuda())


def test_forced_paths_agree(cases):
    _, forest, X, want = cases("classes17")
    for B in (5, len(X)):
        chunked = forest._score(X[:B], walk="chunked")
        split = forest._score(X[:B], walk="split")
        default = forest._score(X[:B])
        for a, b, c in zip(chunked, split, default):
            assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(chunked[0], torch.from_numpy(want).cuda())


def test_constants_match_the_header(ext):
    assert (ext.SPLIT_PREFIX_SLOTS, ext.SPLIT_SLICE_TREES, ext.SPLIT_WALK_ITEMS,
            ext.SPLIT_WG_MAX_ROWS, ext.SPLIT_TILE_BYTES, ext.SPLIT_SCRATCH_BYTES) == (
        F.SPLIT_PREFIX_SLOTS, F.SPLIT_SLICE_TREES, F.SPLIT_WALK_ITEMS, F.SPLIT_WG_MAX_ROWS,
        F.SPLIT_TILE_BYTES, F.SPLIT_SCRATCH_BYTES)
    for f in (64, 5, 45, 46, 300, 1, 2048, 2049):
        assert ext.forest_split_rows_per_wg(f) == F.split_rows_per_wg(f)
    for rows, trees, cap in ((1, 1000, 0), (1, 100, 0), (3, 7, 0), (128, 1000, 0), (65, 100, 5),
                             (256, 3, 0), (256, 1000, 1)):
        assert ext.forest_split_trees_per_slice(rows, trees, cap) == F.split_trees_per_slice(
            rows, trees, cap)


@pytest.mark.parametrize("broken", ["short_leaf_rows", "leaf_values_dtype", "aliased"])
def test_binding_preconditions(ext, cases, broken):
    _, forest, X, _ = cases("classes3")
    B, K, T = 40, forest.n_scores, forest.n_trees
    args = dict(X=X[:B].clone(), leaf_values=forest._leaf_values.clone(),
                leaf_rows=torch.full((T * B,), -3, dtype=torch.int32, device="cuda"),
                scores=torch.full((B, K), -7.25, dtype=torch.float64, device="cuda"),
                labels=torch.full((T * B,), -5, dtype=torch.int32, device="cuda"))
    if broken == "short_leaf_rows":
        args["leaf_rows"] = args["leaf_rows"][: T * B - 1]
    elif broken == "leaf_values_dtype":
        args["leaf_values"] = args["leaf_values"].float()
    elif broken == "aliased":
        args["leaf_rows"] = args["labels"]
    kept = {k: v.clone() for k, v in args.items()}
    with pytest.raises(RuntimeError):
        ext.forest_split_predict(args["X"], forest._split_nodes, forest._first,
                                 args["leaf_values"], forest._baseline, forest.max_tree_nodes,
                                 args["leaf_rows"], args["scores"], args["labels"])
    torch.cuda.synchronize()
    assert all(torch.equal(v.view(torch.uint8), kept[k].view(torch.uint8))
               for k, v in args.items())


def test_graph_replay_equals_eager(ext, cases):
    _, forest, X, _ = cases("classes3")
    B, K = 70, forest.n_scores
    scores, labels = forest._score(X[:B], walk="split")          # warm: loads the kernels
    gs, gl = torch.zeros_like(scores), torch.zeros_like(labels)
    rows = torch.empty(forest.n_trees * B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # records, does not run
        ext.forest_split_predict(X[:B], forest._split_nodes, forest._first,
                                 forest._leaf_values, forest._baseline,
                                 forest.max_tree_nodes, rows, gs, gl)
    for _ in range(3):
        gs.fill_(-7.25)
        gl.fill_(-5)
        rows.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gs, scores) and torch.equal(gl, labels)
