"""The three forest kernels on the hand-built forests of
tests/synthetic_forest.py, against its fp64 oracle bit for bit: every case,
every kernel the case names, every cap and row count of the case, each launch
twice, into outputs over-allocated by rows of poison that must stay."""

import numpy as np
import pytest
import synthetic_forest as S
import torch

pytestmark = pytest.mark.gpu
POISON_SCORE, POISON_LABEL, SPARE = -7.25, -5, 3


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    return hip_ext(required=True)


def _launch(ext, kernel, forest, X, cap):
    """One launch through the binding -> (fp64 [B][K], int32 [B]), the spare
    rows checked."""
    B, K = X.shape[0], forest.n_scores
    out = torch.full((B + SPARE, K), POISON_SCORE, dtype=torch.float64, device="cuda")
    labels = torch.full((B + SPARE,), POISON_LABEL, dtype=torch.int32, device="cuda")
    if kernel == "chunked":
        ext.forest_predict(X, forest._nodes, forest._first, forest._baseline,
                           forest.max_tree_nodes, out, labels, cap)
    elif kernel == "split":
        leaf_rows = torch.full((forest.n_trees * B,), -3, dtype=torch.int32, device="cuda")
        ext.forest_split_predict(X, forest._split_nodes, forest._first, forest._leaf_values,
                                 forest._baseline, forest.max_tree_nodes, leaf_rows, out,
                                 labels, cap[0], cap[1])
    else:
        ext.bagged_forest_predict(X, forest._nodes, forest._first, forest._values,
                                  forest.max_tree_nodes, out, labels, cap[0], cap[1])
    torch.cuda.synchronize()
    assert bool((out[B:] == POISON_SCORE).all()) and bool((labels[B:] == POISON_LABEL).all())
    return out[:B], labels[:B]


def _describe(got, want):
    """Where two score arrays differ, for the assertion's message."""
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    return [(int(r), int(k), float(got[r, k]).hex(), float(want[r, k]).hex())
            for r, k in bad[:8]], len(bad)


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernels_equal_the_oracle_bit_for_bit(ext, name):
    case, want = S.case(name), S.expected(name)
    boosted, bagged = S.predictors(name, "cuda")
    X = torch.from_numpy(case.X).cuda()
    by_rows = {}
    for kernel in case.kernels:
        forest = bagged if kernel == "bagged" else boosted
        scores, classes = want[kernel]
        for B in case.rows[kernel]:
            want_scores = torch.from_numpy(scores[:B]).cuda()
            want_labels = torch.from_numpy(classes[:B].astype(np.int32)).cuda()
            for cap in case.caps[kernel]:
                got = _launch(ext, kernel, forest, X[:B], cap)
                again = _launch(ext, kernel, forest, X[:B], cap)
                where = (name, kernel, B, cap)
                assert torch.equal(got[0], want_scores), (
                    where, _describe(got[0].cpu().numpy(), scores[:B]))
                assert torch.equal(got[1], want_labels), where
                assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), where
                by_rows.setdefault((kernel == "bagged", B), []).append(got)
    # chunked and split run on the same row counts (synthetic_forest._finish), so
    # a group holds both boosted paths under all their caps: the same bits
    for runs in by_rows.values():
        for other in runs[1:]:
            assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1])


def test_predictors_take_the_same_paths(ext):
    """The predictors' own entry points on a case of each family: the default
    walk, the forced ones and the bagged predictor give the oracle's bits."""
    for name in ("every_u_k7", "staging_f257", "largest_tree"):
        case, want = S.case(name), S.expected(name)
        boosted, bagged = S.predictors(name, "cuda")
        B = max(case.rows["split"])
        X = torch.from_numpy(case.X[:B]).cuda()
        scores = torch.from_numpy(want["split"][0][:B]).cuda()
        assert torch.equal(boosted.decision_function(X), scores)
        for walk in set(case.kernels) & {"chunked", "split"}:
            assert torch.equal(boosted.decision_function(X, walk=walk), scores)
        if bagged is not None:
            got = bagged._score(X)
            assert torch.equal(got[0], torch.from_numpy(want["bagged"][0][:B]).cuda())


def test_launcher_rules_match_the_helper(ext):
    for rows, trees in ((1, 700), (3, 771), (4, 260), (16, 64), (256, 8), (256, 100)):
        assert ext.forest_split_trees_per_slice(rows, trees, 0) == S.F.split_trees_per_slice(
            rows, trees)
        assert ext.bagged_trees_per_chunk(rows, trees, 0) == S.F.bagged_trees_per_chunk(
            rows, trees)
    for name in S.EVERY_U + S.STAGING:
        case = S.case(name)
        assert ext.forest_rows_per_wg(case.F, case.K) == S.tile_rows("chunked", case.F, case.K)
        assert ext.forest_split_rows_per_wg(case.F) == S.tile_rows("split", case.F, case.K)
        assert ext.bagged_rows_per_wg(case.F, case.K) == S.tile_rows("bagged", case.F, case.K)
