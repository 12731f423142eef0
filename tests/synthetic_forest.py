"""Forests built by hand for the limits of the three forest kernels, and an
fp64 oracle that walks them, shared by tests/test_synthetic_forest_cpu.py and
tests/test_gpu_forest_synthetic.py.

A tree is described independently of any packing (``Tree``), with its nodes in
PREORDER, so the packers' breadth-first renumbering has work to do. The
adapters hand such trees to the production packers (``_pack_tree``,
``_pack_split_tree``, ``_pack_bagged_tree``) in the form sklearn's trees have
and call the predictors' constructors as ``from_sklearn`` does. The oracle
(``oracle_boosted``, ``oracle_bagged``) is written on the description alone: it
widens x to fp64 and compares with the fp64 threshold, and shares no code with
``unionml_amd.ops.forest``.

``CASES`` is the table of forests; ``case(name)`` builds one (cached). Every
tree has two children at each inner node, as the packed formats require, so a
tree's node count is odd: where a limit is an even number (an LDS prefix of P
nodes) the table takes the odd sizes on both sides of it.
"""

import dataclasses
import functools
import types
import zlib

import numpy as np

from unionml_amd.ops import forest as F

FLT_MAX = float(np.finfo(np.float32).max)
SHAPES = ("balanced", "left_chain", "right_chain", "random")
SMALL_SIZES = (31, 7, 1, 15, 3, 29)      # node counts of the "small" trees
ITERATIONS = 3                           # boosting iterations unless a case is about them
PIPELINE_DEPTHS = (1, 7, 8, 9, 16, 17, 25)


# ---------------------------------------------------------------------------
# the tree description
# ---------------------------------------------------------------------------

@dataclasses.dataclass
class Tree:
    """One tree, root at node 0. ``left`` / ``right`` are -1, ``feature`` -2
    and ``threshold`` -2.0 on a leaf (sklearn's conventions); ``value`` is
    fp64 [n] (boosted) or [n][K] (bagged) and holds junk on inner nodes."""
    feature: np.ndarray
    threshold: np.ndarray
    missing_left: np.ndarray
    left: np.ndarray
    right: np.ndarray
    is_leaf: np.ndarray
    value: np.ndarray

    def __len__(self):
        return len(self.left)


def _structure(rng, shape, n):
    """Children of a tree of n nodes (odd) in preorder: the subtree of node i
    with s nodes is [i, i + s), its left child i + 1. Built level by level."""
    assert n % 2 == 1 and shape in SHAPES
    left, right = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    at, size = np.zeros(1, np.int64), np.array([n], np.int64)
    while at.size:
        inner = size > 1
        i, s = at[inner], size[inner]
        if shape == "balanced":
            ls = ((s - 1) // 2) | 1
        elif shape == "left_chain":
            ls = s - 2
        elif shape == "right_chain":
            ls = np.ones_like(s)
        else:
            ls = 2 * rng.randint(0, (s - 1) // 2) + 1 if s.size else s
        left[i], right[i] = i + 1, i + 1 + ls
        at, size = np.concatenate([i + 1, i + 1 + ls]), np.concatenate([ls, s - 1 - ls])
    return left, right


def column_center(f):
    """Where column f of the probe rows is centred, so that a column read in
    another's place changes decisions."""
    return ((np.asarray(f) * 7) % 11 - 5) * 0.5


def near_median(rng, features):
    return column_center(features) + 0.3 * rng.randn(len(features))


def mixed_values(rng, shape):
    """Leaf values across thirteen decades, so that the order of an fp64 sum
    shows in its bits."""
    return rng.randn(*shape) * 10.0 ** rng.randint(-6, 7, shape)


class FeatureDraw:
    """Features for the inner nodes of a forest's trees, in the order asked
    for. "random": uniform; "cover": every feature 0..F-1 once first, then
    uniform with a quarter of the draws on F-1; "last": always F-1."""

    def __init__(self, rng, n_features, mode="random"):
        assert mode in ("random", "cover", "last")
        self.rng, self.F, self.mode = rng, n_features, mode
        self.pending = rng.permutation(n_features) if mode == "cover" else np.zeros(0, np.int64)

    def __call__(self, n):
        if self.mode == "last":
            return np.full(n, self.F - 1, np.int64)
        out = self.rng.randint(0, self.F, n).astype(np.int64)
        if self.mode == "cover":
            out[self.rng.rand(n) < 0.25] = self.F - 1
            take = min(n, len(self.pending))
            out[:take] = self.pending[:take]
            self.pending = self.pending[take:]
        return out


def make_tree(rng, shape, n_nodes, features, K=None, thresholds=near_median,
              values=mixed_values):
    """A tree of ``n_nodes`` nodes in ``shape``: features from ``features(n)``,
    thresholds from ``thresholds(rng, features)``, leaf values from
    ``values(rng, shape)``; K=None: one fp64 a leaf, otherwise a K-vector."""
    left, right = _structure(rng, shape, n_nodes)
    leaf = left < 0
    feature = np.full(n_nodes, -2, np.int64)
    feature[~leaf] = features(int((~leaf).sum()))
    threshold = np.full(n_nodes, -2.0)
    threshold[~leaf] = thresholds(rng, feature[~leaf])
    missing_left = (rng.rand(n_nodes) < 0.5) & ~leaf
    value = np.full((n_nodes,) if K is None else (n_nodes, K), 1e300)
    value[leaf] = values(rng, value[leaf].shape)
    return Tree(feature, threshold, missing_left, left, right, leaf, value)


def as_bagged(rng, tree, K, values=mixed_values):
    """The same tree with a K-vector on every leaf."""
    value = np.full((len(tree), K), 1e300)
    value[tree.is_leaf] = values(rng, (int(tree.is_leaf.sum()), K))
    return dataclasses.replace(tree, value=value)


def stump(feature, threshold, missing_left, left_value, right_value):
    """Root, left leaf, right leaf."""
    v = np.stack([np.full_like(np.asarray(left_value, np.float64), 1e300),
                  np.asarray(left_value, np.float64), np.asarray(right_value, np.float64)])
    return Tree(np.array([feature, -2, -2]), np.array([threshold, -2.0, -2.0]),
                np.array([missing_left, False, False]), np.array([1, -1, -1]),
                np.array([2, -1, -1]), np.array([False, True, True]), v)


# ---------------------------------------------------------------------------
# the oracle: no code of unionml_amd.ops.forest
# ---------------------------------------------------------------------------

def _reach(tree, X64):
    """The leaf (node index in the description) each fp64 row reaches."""
    rows = np.arange(len(X64))
    at = np.zeros(len(X64), np.int64)
    while True:
        inner = ~tree.is_leaf[at]
        if not inner.any():
            return at
        x = X64[rows, np.where(inner, tree.feature[at], 0)]
        with np.errstate(invalid="ignore"):
            go_left = np.where(np.isnan(x), tree.missing_left[at], x <= tree.threshold[at])
        at = np.where(inner, np.where(go_left, tree.left[at], tree.right[at]), at)


def _widen(X):
    return np.asarray(X, dtype=np.float32).astype(np.float64)


def oracle_boosted(trees, baseline, K, X):
    """-> (scores fp64 [B][K], class indices [B]): (0 + baseline[k]), then the
    leaf of tree it * K + k added to column k, one fp64 addition a tree in
    iteration order; the first largest score, or score > 0 at K == 1."""
    X64 = _widen(X)
    scores = np.zeros((len(X64), K)) + np.asarray(baseline, np.float64)
    for t, tree in enumerate(trees):
        scores[:, t % K] = scores[:, t % K] + tree.value[_reach(tree, X64)]
    labels = (scores[:, 0] > 0).astype(np.int64) if K == 1 else scores.argmax(axis=1)
    return scores, labels


def oracle_bagged(trees, K, X):
    """-> (means fp64 [B][K], class indices [B]): the leaves' vectors added in
    tree order from zero, divided once by the tree count; the first largest."""
    X64 = _widen(X)
    acc = np.zeros((len(X64), K))
    for tree in trees:
        acc = acc + tree.value[_reach(tree, X64)]
    acc = acc / float(len(trees))
    return acc, acc.argmax(axis=1)


# ---------------------------------------------------------------------------
# adapters: the description -> sklearn's forms -> the production packers
# ---------------------------------------------------------------------------

# the fields of sklearn's HistGradientBoosting predictor nodes that the packers read
_HGB_NODE = np.dtype([("value", "<f8"), ("feature_idx", "<i8"), ("num_threshold", "<f8"),
                      ("missing_go_to_left", "u1"), ("left", "<u4"), ("right", "<u4"),
                      ("is_leaf", "u1")])


def hgb_nodes(tree):
    """The tree as sklearn's TreePredictor.nodes (a leaf's links are 0)."""
    leaf = tree.is_leaf
    out = np.zeros(len(tree), _HGB_NODE)
    out["value"] = tree.value
    out["feature_idx"] = np.where(leaf, 0, tree.feature)
    out["num_threshold"] = np.where(leaf, 0.0, tree.threshold)
    out["missing_go_to_left"] = tree.missing_left
    out["left"] = np.where(leaf, 0, tree.left)
    out["right"] = np.where(leaf, 0, tree.right)
    out["is_leaf"] = leaf
    return out


def sklearn_tree(tree):
    """The tree with the attributes of sklearn's ``Tree`` that the bagged
    packer reads."""
    return types.SimpleNamespace(
        children_left=tree.left, children_right=tree.right, threshold=tree.threshold,
        feature=tree.feature, value=tree.value[:, None, :],
        missing_go_to_left=tree.missing_left.astype(np.uint8), node_count=len(tree))


def _tree_first(trees):
    return np.concatenate([[0], np.cumsum([len(t) for t in trees])]).astype(np.int32)


def boosted_predictor(trees, baseline, n_features, device="cpu"):
    """ForestPredictor of the trees, assembled as ``from_sklearn`` does."""
    nodes = [hgb_nodes(t) for t in trees]
    chunked = (np.concatenate([F._pack_tree(n) for n in nodes])
               if max(len(n) for n in nodes) <= F.CHUNK_NODES else None)
    packed, first_leaf_row = [], 0
    for n in nodes:
        packed.append(F._pack_split_tree(n, first_leaf_row))
        first_leaf_row += len(packed[-1][1])
    return F.ForestPredictor(chunked, _tree_first(trees),
                             0.0 + np.asarray(baseline, np.float64), n_features,
                             np.concatenate([p[0] for p in packed]),
                             np.concatenate([p[1] for p in packed]), device=device)


def bagged_predictor(trees, n_features, device="cpu"):
    """BaggedForestPredictor of the trees, assembled as ``from_sklearn`` does."""
    packed, first_leaf_row = [], 0
    for t in trees:
        packed.append(F._pack_bagged_tree(sklearn_tree(t), first_leaf_row))
        first_leaf_row += len(packed[-1][1])
    return F.BaggedForestPredictor(np.concatenate([p[0] for p in packed]), _tree_first(trees),
                                   np.concatenate([p[1] for p in packed]), n_features,
                                   device=device)


def from_hgb(est):
    """A fitted HistGradientBoosting estimator -> (trees, baseline, K)."""
    trees = []
    for iteration in est._predictors:
        for predictor in iteration:
            n = predictor.nodes
            leaf = n["is_leaf"].astype(bool)
            trees.append(Tree(np.where(leaf, -2, n["feature_idx"].astype(np.int64)),
                              n["num_threshold"].astype(np.float64),
                              n["missing_go_to_left"].astype(bool) & ~leaf,
                              np.where(leaf, -1, n["left"].astype(np.int64)),
                              np.where(leaf, -1, n["right"].astype(np.int64)), leaf,
                              n["value"].astype(np.float64)))
    baseline = np.asarray(est._baseline_prediction, np.float64).reshape(-1)
    return trees, baseline, len(est._predictors[0])


def from_bagged(est):
    """A fitted random forest / extra-trees / decision tree -> (trees, K)."""
    trees = []
    for e in getattr(est, "estimators_", [est]):
        t = e.tree_
        leaf = t.children_left < 0
        missing = getattr(t, "missing_go_to_left", None)
        missing = np.zeros(t.node_count, bool) if missing is None else missing.astype(bool)
        trees.append(Tree(t.feature.astype(np.int64), t.threshold.astype(np.float64),
                          missing & ~leaf, t.children_left.astype(np.int64),
                          t.children_right.astype(np.int64), leaf,
                          t.value[:, 0, :].astype(np.float64)))
    return trees, trees[0].value.shape[1]


# ---------------------------------------------------------------------------
# the launcher rules that ops/forest.py has no copy of
# ---------------------------------------------------------------------------

def pow2ceil(n):
    p = 1
    while p < n:
        p *= 2
    return p


def pow2floor(n):
    return pow2ceil(n + 1) // 2


def chunked_trees_per_chunk(max_tree_nodes, cap=0):
    """forest_trees_per_chunk of hip/forest.h."""
    n = min(F.CHUNK_NODES // max_tree_nodes, F.CHUNK_TREES)
    return min(n, cap) if cap > 0 else n


def chunked_items(n_features, n_scores):
    """U of forest_predict_kernel<U>."""
    return -(-F.rows_per_wg(n_features, n_scores) * n_scores // F.BLOCK)


def split_rows(n_rows, n_features):
    """R of a split-walk launch of n_rows rows."""
    return min(pow2ceil(n_rows), F.split_rows_per_wg(n_features))


def split_prefix(n_trees_per_slice, max_tree_nodes, prefix_nodes=-1):
    """P of forest_split_walk_kernel."""
    p = min(max_tree_nodes, F.SPLIT_PREFIX_SLOTS, pow2floor(F.SPLIT_PREFIX_SLOTS // n_trees_per_slice))
    return min(p, prefix_nodes) if prefix_nodes >= 0 else p


def bagged_prefix(n_trees_per_chunk, max_tree_nodes, prefix_nodes=-1):
    """P of bagged_forest_predict_kernel (2,048 prefix slots)."""
    p = min(max_tree_nodes, 2048, pow2floor(2048 // n_trees_per_chunk))
    return min(p, prefix_nodes) if prefix_nodes >= 0 else p


def split_sum_rows(n_scores):
    """Rows per workgroup of forest_split_sum_kernel."""
    return pow2floor(F.BLOCK // n_scores)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

DEFAULT_CAPS = {"chunked": (0, 5),                  # trees_per_chunk
                "split": ((-1, 0), (3, 5)),         # (prefix_nodes, trees_per_slice)
                "bagged": ((-1, 0), (3, 5))}        # (prefix_nodes, trees_per_chunk)


@dataclasses.dataclass
class Case:
    name: str
    F: int
    K: int
    kernels: tuple              # of "chunked", "split", "bagged"
    boosted: list               # trees with one fp64 a leaf, len % K == 0 (or None)
    baseline: np.ndarray
    bagged: list                # trees with a K-vector a leaf (or None)
    rows: dict                  # kernel -> row counts B
    caps: dict                  # kernel -> the caps to run under
    X: np.ndarray               # fp32 [max B][F]

    def max_tree_nodes(self, kernel):
        return max(len(t) for t in (self.bagged if kernel == "bagged" else self.boosted))


def tile_rows(kernel, n_features, n_scores):
    return {"chunked": F.rows_per_wg(n_features, n_scores),
            "split": F.split_rows_per_wg(n_features),
            "bagged": F.bagged_rows_per_wg(n_features, n_scores)}[kernel]


def around(R):
    return tuple(sorted({1, R - 1, R + 1, 2 * R + 3}))


def make_rows(rng, n, n_features, trees, nan_share=0.1):
    """n fp32 rows: column f normal around column_center(f), NaN sprinkled
    (more of it in the last column), a row of -inf, of +inf and of NaN, and
    for up to 32 thresholds of the trees the fp32 nearest the threshold and
    its two fp32 neighbours in that column."""
    X = (column_center(np.arange(n_features)) + rng.randn(n, n_features)).astype(np.float32)
    X[rng.rand(n, n_features) < nan_share] = np.nan
    X[rng.rand(n) < 0.3, n_features - 1] = np.nan
    if n > 8:
        X[1], X[2], X[3] = -np.inf, np.inf, np.nan
    inner = [(t.feature[~t.is_leaf], t.threshold[~t.is_leaf]) for t in trees]
    feature = np.concatenate([f for f, _ in inner])
    threshold = np.concatenate([t for _, t in inner])
    pick = rng.permutation(len(feature))[:max(0, min(32, (n - 4) // 3))]
    for i, p in enumerate(pick):
        with np.errstate(over="ignore"):
            x0 = np.float32(threshold[p])
        X[4 + 3 * i: 7 + 3 * i, feature[p]] = [x0, np.nextafter(x0, np.float32(np.inf)),
                                               np.nextafter(x0, np.float32(-np.inf))]
    return X


def _finish(name, rng, n_features, K, kernels, boosted=None, bagged=None, baseline=None,
            rows=None, caps=None, X=None):
    rows = dict(rows or {})
    for kernel in kernels:
        rows.setdefault(kernel, around(tile_rows(kernel, n_features, K)))
    if "chunked" in kernels and "split" in kernels:     # the two boosted paths on the same rows
        rows["chunked"] = rows["split"] = tuple(sorted(set(rows["chunked"]) | set(rows["split"])))
    if boosted is not None and baseline is None:
        baseline = mixed_values(rng, (K,))
    if X is None:
        X = make_rows(rng, max(max(r) for r in rows.values()), n_features,
                      (boosted or []) + (bagged or []))
    assert all(max(r) <= len(X) for r in rows.values())
    assert boosted is None or len(boosted) % K == 0
    return Case(name, n_features, K, tuple(kernels), boosted, baseline, bagged, rows,
                {**DEFAULT_CAPS, **(caps or {})}, X)


def _small_trees(rng, n_trees, draw, sizes=SMALL_SIZES, **kw):
    return [make_tree(rng, SHAPES[(t // 2) % 4], sizes[t % len(sizes)], draw, **kw)
            for t in range(n_trees)]


def _every_u(K):
    def build(name, rng):
        trees = _small_trees(rng, ITERATIONS * K, FeatureDraw(rng, 64))
        return _finish(name, rng, 64, K, ("chunked", "split"), boosted=trees)
    return build


def _staging(n_features):
    """Chains that carry every column, and rows that walk them to the end, so
    that rows MEET the nodes at any F. Column f has a base value b[f] near its
    centre. The even trees are left chains that share the columns 0..F-2 out
    among them, with thresholds a little above b[f]; the odd trees are right
    chains that share them out again, with thresholds a little below. Every
    chain ends in two nodes on column F-1, the first with the missing_left
    value that keeps a NaN on the chain, the second with the other. A row that
    holds b (a "path row") takes every chain to its end, and a column read in
    another's place takes it off some chain unless the two bases lie within a
    threshold's margin. Row 0 is a path row with NaN in column F-1, so the lone
    row of B = 1 reads every column and decides a NaN at F-1 under both
    missing_left values; row 4 is one with a number there; row 5 and two rows
    in three from row 6 on are path rows with up to three columns knocked off;
    the other rows are make_rows' (noise, -inf, +inf, NaN, threshold probes)."""
    def build(name, rng):
        K, n_trees, last = 2, ITERATIONS * 2, n_features - 1
        base = near_median(rng, np.arange(n_features))
        shares = [np.array_split(rng.permutation(last), n_trees // 2) for _ in range(2)]
        trees = []
        for t in range(n_trees):
            down_left = t % 2 == 0
            features = np.concatenate([shares[t % 2][t // 2], [last, last]]).astype(np.int64)

            def thresholds(rng, f, sign=1.0 if down_left else -1.0):
                return base[f] + sign * rng.uniform(0.001, 0.05, len(f))

            tree = make_tree(rng, "left_chain" if down_left else "right_chain",
                             2 * len(features) + 1, lambda n: features, thresholds=thresholds)
            inner = np.flatnonzero(~tree.is_leaf)          # in chain order
            assert np.array_equal(tree.feature[inner], features)
            tree.missing_left[inner[-2:]] = [down_left, not down_left]
            trees.append(tree)

        def path_row(stray=0):
            x = (base + rng.uniform(-0.0005, 0.0005, n_features)).astype(np.float32)
            x[rng.randint(0, n_features, stray)] += np.float32(1.5) * rng.choice([-1, 1], stray)
            return x

        case = _finish(name, rng, n_features, K, ("chunked", "split", "bagged"), boosted=trees,
                       bagged=[as_bagged(rng, t, K) for t in trees])
        case.X[0], case.X[4], case.X[5] = path_row(), path_row(), path_row(stray=3)
        case.X[0, last] = np.nan
        for r in range(6, len(case.X)):
            if r % 3 != 2:
                case.X[r] = path_row(stray=r % 4)
        return case
    return build


def _full_tables(K, n_trees):
    """Stumps and root-only trees, enough of them to fill the three 256-entry
    tables and to go round them."""
    def build(name, rng):
        n_features = 3
        draw = FeatureDraw(rng, n_features)
        trees = [make_tree(rng, "balanced", 1 if t % 5 == 4 else 3, draw) for t in range(n_trees)]
        rows = {"chunked": (1, 3, 2 * F.rows_per_wg(n_features, K) + 3),
                "split": (1, 3, 2 * F.split_rows_per_wg(n_features) + 3),
                "bagged": (1, 3, 2 * F.bagged_rows_per_wg(n_features, K) + 3)}
        return _finish(name, rng, n_features, K, ("chunked", "split", "bagged"), boosted=trees,
                       bagged=[as_bagged(rng, t, K) for t in trees], rows=rows)
    return build


def _multi_chunk(K, n_trees):
    def build(name, rng):
        draw = FeatureDraw(rng, 5, "cover")
        trees = _small_trees(rng, n_trees, draw, K=K)
        return _finish(name, rng, 5, K, ("bagged",), bagged=trees)
    return build


@functools.lru_cache(maxsize=None)
def _pipeline_trees(K):
    """25 iterations of K seven-node trees, and 25 bagged trees, for the
    pipeline cases of K, which take the first ones of each."""
    rng = np.random.RandomState(1000 + K)
    draw = FeatureDraw(rng, 3)
    n = max(PIPELINE_DEPTHS)
    boosted = _small_trees(rng, n * K, draw, sizes=(7, 5, 3))
    bagged = _small_trees(rng, n, draw, sizes=(7, 5, 3), K=K)
    return boosted, bagged, mixed_values(rng, (K,))


def _pipeline(K, depth):
    def build(name, rng):
        boosted, bagged, baseline = _pipeline_trees(K)
        sums = around(split_sum_rows(K))
        caps = {}
        if depth == max(PIPELINE_DEPTHS):      # the longest forest also under every depth as a cap
            caps["bagged"] = DEFAULT_CAPS["bagged"] + tuple((-1, d) for d in PIPELINE_DEPTHS[:-1])
        return _finish(name, rng, 3, K, ("chunked", "split", "bagged"),
                       boosted=boosted[:depth * K], bagged=bagged[:depth], baseline=baseline,
                       rows={"chunked": sums, "split": sums}, caps=caps)
    return build


def _full_chunk(big, shapes):
    """Trees of ``big`` nodes in each of ``shapes`` between small ones."""
    def build(name, rng):
        n_features, K = 4, 2
        draw = FeatureDraw(rng, n_features, "cover")
        trees = _small_trees(rng, 2, draw)
        for shape in shapes:
            trees.append(make_tree(rng, shape, big, draw))
            trees += _small_trees(rng, 2, draw)
        trees += _small_trees(rng, len(trees) % K, draw)
        return _finish(name, rng, n_features, K, ("chunked", "split"), boosted=trees)
    return build


def _prefix(sizes, n_trees, rows):
    def build(name, rng):
        n_features, K = 6, 2
        draw = FeatureDraw(rng, n_features, "cover")
        trees = []
        for t in range(n_trees):
            n = sizes[t % len(sizes)]       # chains only where they stay shallow
            shape = SHAPES[(t // 3) % 4] if n < 600 else ("random" if t % 2 else "balanced")
            trees.append(make_tree(rng, shape, n, draw))
        zero = ((-1, 0), (0, 0), (3, 5))
        return _finish(name, rng, n_features, K, ("split", "bagged"), boosted=trees,
                       bagged=[as_bagged(rng, t, K) for t in trees],
                       rows={"split": rows, "bagged": rows}, caps={"split": zero, "bagged": zero})
    return build


def _largest(name, rng):
    n_features, K = 7, 1
    draw = FeatureDraw(rng, n_features)
    trees = [make_tree(rng, "balanced", 7, draw),
             make_tree(rng, "balanced", F.SPLIT_MAX_TREE_NODES - 1, draw),
             make_tree(rng, "random", 5, draw)]
    return _finish(name, rng, n_features, K, ("split", "bagged"), boosted=trees,
                   bagged=[as_bagged(rng, t, K) for t in trees],
                   rows={"split": (5,), "bagged": (5,)})


COMPARE_THRESHOLDS = tuple(s * t for t in (0.0, 2.0 ** -149, 2.0 ** -126, 1e-50, 1e39, FLT_MAX,
                                           np.inf) for s in (1.0, -1.0)) + (0.1,)
COMPARE_INPUTS = np.array(
    [s * x for x in (0.0, 2.0 ** -149, 2.0 ** -126, FLT_MAX, np.inf) for s in (1.0, -1.0)]
    + [np.nan, np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(1))], dtype=np.float32)


def _compare(name, rng):
    """One stump a (threshold, missing_left) on the only feature; the left
    leaf of stump i holds 2^i and the right one 0, so a row's score spells
    out the stumps that sent it left."""
    K = 2
    stumps = [(t, m) for t in COMPARE_THRESHOLDS for m in (False, True)]
    boosted = [stump(0, t, m, 2.0 ** (i // K), 0.0) for i, (t, m) in enumerate(stumps)]
    bagged = [stump(0, t, m, [2.0 ** i, 1.0], [0.0, 3.0]) for i, (t, m) in enumerate(stumps)]
    X = COMPARE_INPUTS[:, None].copy()
    rows = (len(X),)
    return _finish(name, rng, 1, K, ("chunked", "split", "bagged"), boosted=boosted,
                   bagged=bagged, baseline=np.zeros(K), X=X,
                   rows={"chunked": rows, "split": rows, "bagged": rows})


# Leaf values in tree order whose fp64 sum from zero has other bits under every
# cyclic rotation (tests/test_synthetic_forest_cpu.py holds that)
ORDER_A = (2.0 ** 53, 1.0, 1.0, -2.0 ** 53, 2.0 ** 53, 1e-3, 2.0 ** -30, 1.0, 3.0, 1.0,
           2.0 ** 53 + 2.0, 3.0, -2.0 ** 53, -2.0 ** 53, -2.0 ** 60, 2.0 ** 60, 0.1, 1.0, 1.0,
           2.0 ** -30)
ORDER_B = (2.0 ** 53, 1.0, 1.0, -2.0 ** 53, 2.0 ** -30, 1.0, 1e-3, 0.1, 2.0 ** 53, 1.0, 1.0,
           1e-3, -2.0 ** 53, 3.0, 1.0, -1.0, -2.0 ** 60, 1.0, 2.0 ** 60, -1.0)
ORDER_TINY = (-0.0, 5e-324, 5e-324, -0.0)      # and a baseline of -0.0: the sum is 1e-323


def ordered_sum(values, start=0.0):
    acc = np.float64(start)
    for v in values:
        acc = acc + np.float64(v)
    return acc


def _order(left, right, baseline):
    """Stumps on feature 0 whose left leaves hold ``left`` and right leaves
    ``right`` in tree order: the row of -inf adds ``left``, the row of +inf
    ``right``, the others a mixture."""
    def build(name, rng):
        thresholds = near_median(rng, np.zeros(len(left), np.int64))
        boosted = [stump(0, t, bool(i % 2), a, b)
                   for i, (a, b, t) in enumerate(zip(left, right, thresholds))]
        bagged = [dataclasses.replace(t, value=t.value[:, None].copy()) for t in boosted]
        rows = {k: (1, 19) for k in ("chunked", "split", "bagged")}
        return _finish(name, rng, 2, 1, ("chunked", "split", "bagged"), boosted=boosted,
                       bagged=bagged, baseline=np.array([baseline]), rows=rows)
    return build


CASES = {}
for _K in (2, 3, 5, 7, 10, 12, 14, 16):
    CASES[f"every_u_k{_K}"] = _every_u(_K)
for _F in (1, 2, 3, 128, 255, 256, 257, 511, 512, 1024, 2047, 2048):
    CASES[f"staging_f{_F}"] = _staging(_F)
CASES["full_tables_k1"] = _full_tables(1, 700)
CASES["full_tables_k3"] = _full_tables(3, 771)      # 257 iterations: a chunk boundary inside one
CASES["multi_chunk_k2"] = _multi_chunk(2, 100)
CASES["multi_chunk_k32"] = _multi_chunk(32, 40)
for _K in (1, 3, 5, 17, 32):
    for _D in PIPELINE_DEPTHS:
        CASES[f"pipeline_k{_K}_d{_D}"] = _pipeline(_K, _D)
CASES["full_chunk_2047"] = _full_chunk(2047, ("balanced", "left_chain", "right_chain"))
CASES["full_chunk_1023"] = _full_chunk(1023, ("left_chain", "random"))
CASES["full_chunk_1025"] = _full_chunk(1025, ("right_chain", "random"))
# sizes around the prefix P of the split walk (4,096 slots over S trees) and of
# the bagged kernel (2,048 over C): S = C = 256 gives P = 16 and 8, S = C = 64
# gives 64 and 32, full row tiles (S = 4, C = 8) give 1,024 and 256
CASES["prefix_s256"] = _prefix((7, 9, 15, 17, 19, 31, 33, 63, 65), 260, (1, 3))
CASES["prefix_s64"] = _prefix((31, 33, 35, 63, 65, 67, 127, 129, 255, 257), 64, (16,))
CASES["prefix_s4"] = _prefix((255, 257, 259, 1023, 1025, 1027, 4095, 4097), 8, (515,))
CASES["largest_tree"] = _largest
CASES["compare_table"] = _compare
CASES["order_probe"] = _order(ORDER_A, ORDER_B, 0.0)
CASES["order_probe_tiny"] = _order(ORDER_TINY, ORDER_TINY[::-1], -0.0)
del _K, _F, _D

EVERY_U = [n for n in CASES if n.startswith("every_u")]
STAGING = [n for n in CASES if n.startswith("staging")]
FULL_TABLES = [n for n in CASES if n.startswith("full_tables")]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name](name, np.random.RandomState(zlib.crc32(name.encode())))


@functools.lru_cache(maxsize=None)
def predictors(name, device="cpu"):
    """-> (ForestPredictor or None, BaggedForestPredictor or None) of a case."""
    c = case(name)
    return (None if c.boosted is None else boosted_predictor(c.boosted, c.baseline, c.F, device),
            None if c.bagged is None else bagged_predictor(c.bagged, c.F, device))


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> kernel -> (fp64 [max B][K], class indices) by the oracle, computed
    once; the boosted kernels share theirs. Callers do not write to them."""
    c = case(name)
    out = {}
    if c.boosted is not None:
        out["chunked"] = out["split"] = oracle_boosted(c.boosted, c.baseline, c.K, c.X)
    if c.bagged is not None:
        out["bagged"] = oracle_bagged(c.bagged, c.K, c.X)
    return out
