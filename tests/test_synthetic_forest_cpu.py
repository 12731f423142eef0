"""The hand-built forests of tests/synthetic_forest.py without a GPU: the
oracle against sklearn bit for bit, the three host walks (and with them the
packers at their field limits) against the oracle bit for bit, and the case
table against the limits it claims to reach."""

import bagged_fixtures
import forest_fixtures
import numpy as np
import pytest
import synthetic_forest as S

from unionml_amd.ops import forest as F


# ---- the oracle is sklearn's arithmetic ---------------------------------------------

@pytest.mark.parametrize("name", ["classes17", "deep", "regressor", "root_only"])
def test_oracle_equals_sklearn_boosted(name):
    est = forest_fixtures.fitted(name)
    X = forest_fixtures.probe_rows(F.ForestPredictor.from_sklearn(est, device="cpu"), 300)
    trees, baseline, K = S.from_hgb(est)
    scores, labels = S.oracle_boosted(trees, baseline, K, X)
    want = forest_fixtures.sklearn_scores(est, X)
    assert np.array_equal(scores, want)
    if hasattr(est, "classes_"):
        assert np.array_equal(est.classes_[labels], forest_fixtures.raw_argmax_labels(est, want))


@pytest.mark.parametrize("name", ["rf_nan", "rf_classes32", "rf_regressor", "stumps"])
def test_oracle_equals_sklearn_bagged(name):
    est = bagged_fixtures.fitted(name)
    forest = F.BaggedForestPredictor.from_sklearn(est, device="cpu")
    X = bagged_fixtures.probe_rows(name, forest, 300)
    trees, K = S.from_bagged(est)
    means, labels = S.oracle_bagged(trees, K, X)
    want = bagged_fixtures.sklearn_means(est, X)
    assert np.array_equal(means, want)
    assert np.array_equal(labels, want.argmax(axis=1))


# ---- the host walks, through the production packers, are the oracle -----------------

@pytest.mark.parametrize("name", sorted(S.CASES))
def test_host_walks_equal_the_oracle(name):
    case, want = S.case(name), S.expected(name)
    boosted, bagged = S.predictors(name)
    if boosted is not None:
        scores, labels = want["split"]
        assert np.array_equal(boosted._walk_split_cpu(case.X), scores)
        if boosted._nodes_np is not None:
            assert np.array_equal(boosted._walk_cpu(case.X)[0], scores)
        else:
            assert "chunked" not in case.kernels
        got = boosted._score(case.X, walk="split")
        assert np.array_equal(got[0].numpy(), scores) and np.array_equal(got[1].numpy(), labels)
    if bagged is not None:
        means, labels = want["bagged"]
        assert np.array_equal(bagged._walk_cpu(case.X), means)
        assert np.array_equal(bagged._score(case.X)[1].numpy(), labels)


def test_trees_are_not_breadth_first():
    tree = S.case("every_u_k5").boosted[0]
    assert len(tree) == 31
    order, _ = F._breadth_first(np.where(tree.is_leaf, 0, tree.left),
                                np.where(tree.is_leaf, 0, tree.right), ~tree.is_leaf)
    assert not np.array_equal(order, np.arange(len(tree)))


# ---- the table reaches what it claims ------------------------------------------------

def test_every_item_count_of_the_chunked_kernel():
    items = {}
    for name in S.EVERY_U:
        case = S.case(name)
        assert F.rows_per_wg(case.F, case.K) == 128
        items[name] = S.chunked_items(case.F, case.K)
    assert sorted(items.values()) == [1, 2, 3, 4, 5, 6, 7, 8]


def _visits(tree, X64):
    """A walk of the description that records itself -> (row, column) pairs
    read, and (row, node) pairs at which a NaN was decided."""
    rows, at = np.arange(len(X64)), np.zeros(len(X64), np.int64)
    read, nan_at = [], []
    while True:
        live = ~tree.is_leaf[at]
        if not live.any():
            return np.concatenate(read), np.concatenate(nan_at)
        r, node = rows[live], at[live]
        x = X64[r, tree.feature[node]]
        read.append(np.stack([r, tree.feature[node]], axis=1))
        nan_at.append(np.stack([r, node], axis=1)[np.isnan(x)])
        with np.errstate(invalid="ignore"):
            go_left = np.where(np.isnan(x), tree.missing_left[node], x <= tree.threshold[node])
        at[live] = np.where(go_left, tree.left[node], tree.right[node])


@pytest.mark.parametrize("name", S.STAGING)
def test_staging_rows_meet_every_column(name):
    """Not only does every column split a node: within the rows of EVERY
    launch (B = 1 included) the walks read every column of the tile, and
    decide a NaN in the last column under both missing_left values."""
    case = S.case(name)
    last, X64 = case.F - 1, case.X.astype(np.float64)
    for trees in (case.boosted, case.bagged):
        visits = [_visits(t, X64) for t in trees]
        for B in sorted({B for kernel in case.kernels for B in case.rows[kernel]}):
            columns, decided = set(), set()
            for tree, (read, nan_at) in zip(trees, visits):
                columns |= set(read[read[:, 0] < B, 1].tolist())
                nodes = nan_at[nan_at[:, 0] < B, 1]
                nodes = nodes[tree.feature[nodes] == last]
                decided |= set(tree.missing_left[nodes].tolist())
            assert columns == set(range(case.F)), (B, len(columns))
            assert decided == {False, True}, B
        # more than one row gets to the bottom of a chain, and not all do
        depth = [len(np.unique(S._reach(t, X64))) for t in trees]
        assert min(depth) >= 2
    if case.F == 2048:
        # the packed bagged node: all eleven feature bits beside the missing bit
        meta = S.predictors(name)[1]._nodes_np["meta"]
        assert (meta & 0xFFF == 0xFFF).any() and (meta & 0xFFF == 0x7FF).any()


def test_staging_takes_both_branches_of_the_column_step():
    wide = [S.case(n).F for n in S.STAGING]
    assert any(256 % f == 0 and f > 1 for f in wide) and {255, 256, 257, 2047, 2048} <= set(wide)
    for kernel in ("chunked", "split", "bagged"):
        assert S.tile_rows(kernel, 2048, 2) == 4 and S.tile_rows(kernel, 2047, 2) == 4


@pytest.mark.parametrize("name", S.FULL_TABLES)
def test_full_tables_are_full(name):
    case = S.case(name)
    boosted, bagged = S.predictors(name)
    T = len(case.boosted)
    assert T > 2 * 256 and T % 256 != 0 and len(case.bagged) == T
    assert S.chunked_trees_per_chunk(boosted.max_tree_nodes) == F.CHUNK_TREES == 256
    for B in (1, 3):
        assert B in case.rows["split"] and B in case.rows["bagged"]
        assert F.split_trees_per_slice(S.split_rows(B, case.F), T) == F.SPLIT_SLICE_TREES == 256
        assert F.bagged_trees_per_chunk(B, T) == F.BAGGED_CHUNK_TREES == 256
    for kernel in case.kernels:
        R = S.tile_rows(kernel, case.F, case.K)
        assert 2 * R + 3 in case.rows[kernel]
    if case.K == 3:
        assert 256 % case.K != 0       # a chunk boundary inside an iteration


def test_natural_multi_chunk():
    c = S.case("multi_chunk_k2")
    R = F.bagged_rows_per_wg(c.F, c.K)
    assert (R, F.bagged_trees_per_chunk(R, len(c.bagged)), -(-len(c.bagged) // 8)) == (256, 8, 13)
    assert 2 * R + 3 in c.rows["bagged"]
    c = S.case("multi_chunk_k32")
    R = F.bagged_rows_per_wg(c.F, c.K)
    assert (R, F.bagged_trees_per_chunk(R, len(c.bagged))) == (64, 32) and len(c.bagged) == 40


def test_pipeline_depths_and_sum_rows():
    assert {S.split_sum_rows(K) for K in (1, 3, 5, 17, 32)} == {256, 64, 32, 8}
    for K in (1, 3, 5, 17, 32):
        for depth in S.PIPELINE_DEPTHS:
            c = S.case(f"pipeline_k{K}_d{depth}")
            assert len(c.boosted) == depth * K and len(c.bagged) == depth
            assert c.rows["split"] == S.around(S.split_sum_rows(K))
            # a lone row walks the whole bagged forest as one chunk
            assert F.bagged_trees_per_chunk(1, depth) == depth
    assert {d % 8 for d in S.PIPELINE_DEPTHS} >= {0, 1, 7} and max(S.PIPELINE_DEPTHS) > 24


def test_full_chunks_and_long_walks():
    boosted, _ = S.predictors("full_chunk_2047")
    case = S.case("full_chunk_2047")
    assert boosted.max_tree_nodes == 2047 and S.chunked_trees_per_chunk(2047) == 1
    assert -(-2047 // F.BLOCK) == 8                 # all eight pieces of a chunk stored
    assert S.chunked_items(case.F, case.K) == 8
    big = [t for t in case.boosted if len(t) == 2047]
    assert len(big) == 3
    X64 = case.X.astype(np.float64)
    for tree in big[1:]:                            # the chains: both ends within the first rows
        depth = _depths(tree)
        assert depth.max() == 1023
        reached = depth[S._reach(tree, X64[:min(case.rows["chunked"][1], case.rows["split"][1])])]
        assert reached.min() == 1 and reached.max() == 1023
    assert (S.chunked_trees_per_chunk(S.predictors("full_chunk_1023")[0].max_tree_nodes),
            S.chunked_trees_per_chunk(S.predictors("full_chunk_1025")[0].max_tree_nodes)) == (2, 1)
    # the 15-bit left offset and the 16-bit feature hold what the cases put there
    meta = boosted._nodes_np["meta"]
    assert ((meta >> 16) & 0x7FFF).max() == 2046


def _depths(tree):
    depth = np.zeros(len(tree), np.int64)
    for i in np.flatnonzero(~tree.is_leaf):         # preorder: a parent before its children
        depth[tree.left[i]] = depth[tree.right[i]] = depth[i] + 1
    return depth


@pytest.mark.parametrize("name,rows,S_,P_split,C_,P_bagged", [
    ("prefix_s256", 1, 256, 16, 256, 8), ("prefix_s256", 3, 256, 16, 256, 8),
    ("prefix_s64", 16, 64, 64, 64, 32), ("prefix_s4", 515, 4, 1024, 8, 256)])
def test_prefix_edges(name, rows, S_, P_split, C_, P_bagged):
    case = S.case(name)
    boosted, bagged = S.predictors(name)
    T, sizes = len(case.boosted), {len(t) for t in case.boosted}
    assert rows in case.rows["split"] and rows in case.rows["bagged"]
    assert F.split_trees_per_slice(S.split_rows(rows, case.F), T) == S_
    assert S.split_prefix(S_, boosted.max_tree_nodes) == P_split
    assert F.bagged_trees_per_chunk(min(rows, bagged.rows_per_wg), T) == C_
    assert S.bagged_prefix(C_, bagged.max_tree_nodes) == P_bagged
    for P in (P_split, P_bagged):
        assert {P - 1, P + 1, 4 * P - 1, 4 * P + 1} <= sizes
    assert (0, 0) in case.caps["split"] and (0, 0) in case.caps["bagged"]


def test_largest_tree():
    case = S.case("largest_tree")
    boosted, bagged = S.predictors("largest_tree")
    assert boosted.max_tree_nodes == bagged.max_tree_nodes == (1 << 20) - 1
    assert boosted._nodes_np is None
    for nodes in (boosted._split_nodes_np, bagged._nodes_np):
        # breadth-first, a child lies at most two levels' width ahead: about
        # half the nodes, which is the largest distance the node limit allows
        assert (nodes["meta"] >> 12).max() == (1 << 19) - 1
    assert case.rows["split"] == case.rows["bagged"] == (5,)


def test_compare_table_holds_the_edges():
    case = S.case("compare_table")
    assert len(S.COMPARE_THRESHOLDS) == 15 and len(case.boosted) == 30
    assert len(case.X) == 13 and case.F == 1
    thr = {np.float64(t.threshold[0]).tobytes() for t in case.boosted}
    assert len(thr) == 15                                  # +0.0 and -0.0 are both there
    # the packed thresholds: below the fp32 range lands on the smallest
    # denormal of that sign or on zero, beyond it on FLT_MAX or -inf
    assert F.rd32(-1e-50) == -np.float32(2.0 ** -149) and F.rd32(1e-50) == 0.0
    assert F.rd32(1e39) == np.float32(S.FLT_MAX) and F.rd32(-1e39) == -np.inf
    # what tells a flushing compare: -0.0 <= -1e-50 is false
    scores, _ = S.expected("compare_table")["split"]
    at = [i for i, t in enumerate(case.boosted) if t.threshold[0] == -1e-50]
    row = int(np.flatnonzero(np.signbit(case.X[:, 0]) & (case.X[:, 0] == 0))[0])
    for i in at:
        assert int(scores[row, i % case.K]) >> (i // case.K) & 1 == 0


@pytest.mark.parametrize("values", [S.ORDER_A, S.ORDER_B])
def test_order_probe_tells_every_rotation(values):
    documented = S.ordered_sum(values)
    assert np.isfinite(documented)
    for k in range(1, len(values)):
        rotated = S.ordered_sum(values[k:] + values[:k])
        assert rotated.tobytes() != documented.tobytes()
        # and so does the bagged kernel's mean, which divides the sum once
        assert (rotated / len(values)).tobytes() != (documented / len(values)).tobytes()
    assert len(values) > 2 * 8                             # three rounds of the ahead-of-8 sum


def test_order_probe_rows_add_the_pure_sequences():
    case = S.case("order_probe")
    scores, _ = S.expected("order_probe")["chunked"]
    assert np.all(case.X[1] == -np.inf) and np.all(case.X[2] == np.inf)
    assert scores[1, 0].tobytes() == S.ordered_sum(S.ORDER_A).tobytes()
    assert scores[2, 0].tobytes() == S.ordered_sum(S.ORDER_B).tobytes()
    tiny, _ = S.expected("order_probe_tiny")["chunked"]
    assert tiny[1, 0] == 1e-323 and not np.signbit(tiny[1, 0])
