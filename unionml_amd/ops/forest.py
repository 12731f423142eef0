"""Device-resident inference of a fitted gradient-boosted forest.

``ForestPredictor.from_sklearn(est)`` packs a fitted
``HistGradientBoostingClassifier`` / ``HistGradientBoostingRegressor`` into
flat tensors (the format of ``hip/forest.h``) and scores rows through
``forest_predict_kernel``. The kernel makes sklearn's comparisons and
sklearn's fp64 additions in sklearn's order, so ``decision_function`` equals
``est.decision_function`` bit for bit (docs/kernels.md "Forest inference").
On a machine without a GPU the same packed arrays are walked by a plain
vectorised fp64 traversal; on a GPU machine a missing extension is the usual
``KernelExtensionNotBuilt``.

Every boosted forest is also packed for the **split walk** (``hip/forest_split.h``,
the bagged 8-byte node and one fp64 per leaf): ``forest_split_walk_kernel``
spreads (row, tree) walks over the whole device and ``forest_split_sum_kernel``
adds their leaves in sklearn's order, so the bits are the same. It serves
small batches, which the chunked kernel walks as one serial chain, and trees
of more than 2,048 nodes, which the chunked kernel cannot hold
(docs/kernels.md "Split walk"). ``walk=`` forces a path, ``walk_for(B)``
tells the choice.

``BaggedForestPredictor`` does the same for ``RandomForest*``, ``ExtraTrees*``
and single ``DecisionTree*`` / ``ExtraTree*`` estimators (the format of
``hip/bagged_forest.h``, ``bagged_forest_predict_kernel``): ``predict_proba``
/ ``predict`` equal sklearn's at ``n_jobs=None`` bit for bit. The module's
``from_sklearn(est)`` returns the predictor that fits the estimator, and
``device_forest(est)`` keeps it on the estimator for the apps. What the two
predictors share (device, upload, input check, output handling) is
``_PackedForest``.
"""

import numpy as np
import torch

from unionml_amd.ops import hip_ext

# the Python copy of hip/forest_limits.h and hip/forest.h (a GPU test holds
# the two equal)
MAX_CLASSES = 32
MAX_FEATURES = 2048
CHUNK_NODES = 2048          # the most nodes one tree may have: one LDS chunk
CHUNK_TREES = 256
MIN_ROWS, MAX_ROWS = 4, 2048
BLOCK, MAX_ITEMS = 256, 8
TILE_BYTES = 80 * 1024 - (CHUNK_NODES * 16 + CHUNK_TREES * 4 + MAX_CLASSES * 8)

NODE_DTYPE = np.dtype([("thr", "<f4"), ("meta", "<u4"), ("value", "<f8")])
META_LEFT_SHIFT, META_MISSING_LEFT = 16, 1 << 31

# the Python copy of hip/forest_split.h (a GPU test holds the two equal)
SPLIT_PREFIX_SLOTS = 4096
SPLIT_SLICE_TREES = 256
SPLIT_WALK_ITEMS = 1024
SPLIT_WG_MAX_ROWS = 256
SPLIT_TILE_BYTES = 80 * 1024 - (SPLIT_PREFIX_SLOTS * 8 + 2 * SPLIT_SLICE_TREES * 4)
SPLIT_SCRATCH_BYTES = 64 << 20      # leaf_rows of one launch; larger calls go in row blocks
SPLIT_MAX_TREE_NODES = 1 << 20      # the bagged node's 20 bits of distance

# Measured (profiles/r17_forest_split.md): the largest benchmarked batch at
# which the split walk beats the chunked kernel on the digits forest by more
# than the spread of the timing windows. walk=None takes the split walk up to
# here.
split_max_rows = 16384


def rd32(t):
    """fp64 thresholds rounded to fp32 towards -inf: for every fp32 ``x``,
    ``x <= t`` (in fp64) holds exactly when ``x <= rd32(t)`` (in fp32)."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = t.astype(np.float32)
    up = f.astype(np.float64) > t          # the conversion rounded up
    return np.where(up, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def _tile_rows(n_features, n_scores, max_rows, tile_bytes, max_items):
    """forest_tile_rows of hip/forest_limits.h: the largest power of two in
    MIN_ROWS..max_rows whose fp32 tile (odd row stride) fits ``tile_bytes``
    and whose rows x scores fit ``max_items``; 0 when F or K is out of range."""
    if not (1 <= n_features <= MAX_FEATURES and 1 <= n_scores <= MAX_CLASSES):
        return 0
    R = max_rows
    while R > MIN_ROWS and (R * (n_features | 1) * 4 > tile_bytes or R * n_scores > max_items):
        R //= 2
    return R


def rows_per_wg(n_features: int, n_scores: int) -> int:
    """Rows per workgroup of the boosted kernel: up to 2,048, rows x classes
    within 8 items a thread."""
    return _tile_rows(n_features, n_scores, MAX_ROWS, TILE_BYTES, BLOCK * MAX_ITEMS)


def split_rows_per_wg(n_features: int) -> int:
    """Rows per workgroup that the split walk's tile allows (a smaller batch
    takes its own size rounded up to a power of two)."""
    return _tile_rows(n_features, 1, SPLIT_WG_MAX_ROWS, SPLIT_TILE_BYTES, SPLIT_WG_MAX_ROWS)


def split_trees_per_slice(rows: int, n_trees: int, cap: int = 0) -> int:
    """Trees a workgroup of the split walk that holds ``rows`` rows owns."""
    rp = 1
    while rp < rows:
        rp *= 2
    n = max(1, min(SPLIT_WALK_ITEMS // rp, SPLIT_SLICE_TREES, n_trees))
    return min(n, cap) if cap > 0 else n


def _breadth_first(left, right, inner):
    """A tree's nodes (root 0, ``inner`` marking those with children) in
    breadth-first order, level by level, so that a node's children end up
    adjacent -> (old index of each new node, new index of each old node)."""
    levels, level = [], np.zeros(1, dtype=np.int64)
    while level.size:
        levels.append(level)
        parents = level[inner[level]]
        level = np.stack([left[parents], right[parents]], axis=1).reshape(-1).astype(np.int64)
    order = np.concatenate(levels)
    assert len(order) == len(inner)
    new_of = np.empty(len(order), dtype=np.int64)
    new_of[order] = np.arange(len(order))
    return order, new_of


def _pack_tree(nodes):
    """One sklearn tree -> packed nodes, renumbered breadth-first; a leaf
    points at itself behind thr = +inf with the missing-goes-left bit set."""
    order, new_of = _breadth_first(nodes["left"], nodes["right"],
                                   ~nodes["is_leaf"].astype(bool))
    src = nodes[order]
    leaf = src["is_leaf"].astype(bool)
    out = np.zeros(len(order), dtype=NODE_DTYPE)
    out["thr"] = np.where(leaf, np.float32(np.inf), rd32(src["num_threshold"]))
    left = np.where(leaf, np.arange(len(order)), new_of[src["left"]])
    assert np.all(leaf | (new_of[src["right"]] == left + 1))
    missing_left = leaf | src["missing_go_to_left"].astype(bool)
    feature = np.where(leaf, 0, src["feature_idx"])
    out["meta"] = (feature.astype(np.uint32) | (left.astype(np.uint32) << META_LEFT_SHIFT)
                   | np.where(missing_left, np.uint32(META_MISSING_LEFT), np.uint32(0)))
    out["value"] = np.where(leaf, src["value"], 0.0)
    return out


def _pack_split_tree(nodes, first_leaf_row):
    """One sklearn boosted tree -> (bagged nodes, leaf values [leaves]),
    renumbered breadth-first; leaves number the rows of leaf_values from
    ``first_leaf_row`` in that order."""
    order, new_of = _breadth_first(nodes["left"], nodes["right"],
                                   ~nodes["is_leaf"].astype(bool))
    src = nodes[order]
    n = len(order)
    leaf = src["is_leaf"].astype(bool)
    dist = np.where(leaf, 0, new_of[np.where(leaf, 0, src["left"])] - np.arange(n))
    assert np.all(leaf | (new_of[src["right"]] == np.arange(n) + dist + 1))
    out = np.zeros(n, dtype=BAGGED_NODE_DTYPE)
    out["thr"] = np.where(leaf, first_leaf_row + np.cumsum(leaf) - 1,
                          rd32(src["num_threshold"]).view(np.uint32))
    out["meta"] = (np.where(leaf, 0, src["feature_idx"]).astype(np.uint32)
                   | np.where(~leaf & src["missing_go_to_left"].astype(bool),
                              np.uint32(BAGGED_META_MISSING_LEFT), np.uint32(0))
                   | (dist.astype(np.uint32) << BAGGED_META_DIST_SHIFT))
    return out, np.ascontiguousarray(src["value"][leaf], dtype=np.float64)


def _leaves_cpu(nodes, tree_first, X, t):
    """leaf_values rows that the rows of X reach in tree t of a forest of
    bagged nodes, by a vectorised walk."""
    thr_bits, meta = nodes["thr"], nodes["meta"]
    thr = thr_bits.view(np.float32)
    rows = np.arange(X.shape[0])
    idx = np.full(X.shape[0], int(tree_first[t]))
    while True:
        m = meta[idx]
        dist = (m >> BAGGED_META_DIST_SHIFT).astype(np.int64)
        x = X[rows, m & 0x7FF]
        with np.errstate(invalid="ignore"):
            go_left = np.where(np.isnan(x), (m & BAGGED_META_MISSING_LEFT) != 0,
                               x <= thr[idx])
        if not dist.any():
            return thr_bits[idx].astype(np.int64)
        idx = idx + np.where(dist > 0, dist + np.where(go_left, 0, 1), 0)


class _PackedForest:
    """What the two predictors do alike: a packed forest's nodes and tree
    table on one device, the check of the rows, and the outputs around the
    kernel (or, without a GPU, around the host walk). A predictor adds its
    own third array, ``_launch`` (the kernel) and ``_host`` (the walk)."""

    def __init__(self, nodes, tree_first, n_features, n_scores, classes, device):
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.n_features = int(n_features)
        self.n_scores = int(n_scores)
        self.n_trees = int(len(tree_first) - 1)
        self.max_tree_nodes = int(np.diff(tree_first).max())
        self.classes_ = None if classes is None else np.asarray(classes)
        self._nodes_np, self._first_np = nodes, tree_first
        self._ext = None
        self._nodes = None
        if self.device.type == "cuda":
            self._ext = hip_ext(required=True)
            self._nodes = self._upload_nodes(nodes)
            self._first = torch.from_numpy(tree_first).to(self.device)

    def _upload(self, array):
        """The predictor's own array on the device (None without a GPU)."""
        return None if self._ext is None else torch.from_numpy(array).to(self.device)

    def _upload_nodes(self, nodes):
        """Packed nodes as int32 words [N][words] on the device (None without
        a GPU, or for a packing the forest does not have)."""
        if self._ext is None or nodes is None:
            return None
        words = nodes.dtype.itemsize // 4
        return self._upload(nodes.view("<i4").reshape(-1, words))

    @staticmethod
    def _refuse_beyond_limits(K, what, F, n_nodes):
        """The refusals of ``from_sklearn`` that both kernels share."""
        if not 1 <= K <= MAX_CLASSES:
            raise ValueError(f"{K} {what}: the kernel takes 1..{MAX_CLASSES}")
        if F > MAX_FEATURES:
            raise ValueError(f"{F} features: the row tile takes at most {MAX_FEATURES}")
        if n_nodes > 1 << 30:
            raise ValueError("the forest has more than 2^30 nodes")

    def _rows(self, X):
        if hasattr(X, "tocsr"):
            raise ValueError("a sparse X is not supported: pass a dense float [B][F]")
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X))
        if X.dim() != 2 or X.shape[1] != self.n_features or not X.is_floating_point():
            raise ValueError(f"X must be a float [B][{self.n_features}], is {tuple(X.shape)} "
                             f"{X.dtype}")
        return X.to(self.device, torch.float32).contiguous()

    def _run(self, X, *caps):
        """-> (fp64 [B][K], class indices int32 [B]) on the device, from the
        kernel under ``caps`` or from the host walk."""
        X = self._rows(X)
        B = X.shape[0]
        out = torch.empty(B, self.n_scores, dtype=torch.float64, device=self.device)
        labels = torch.empty(B, dtype=torch.int32, device=self.device)
        if B == 0:
            return out, labels
        if self._ext is not None:
            self._launch(X, out, labels, *caps)
            return out, labels
        values, idx = self._host(X.numpy(), *caps)
        out.copy_(torch.from_numpy(values))
        labels.copy_(torch.from_numpy(idx.astype(np.int32)))
        return out, labels


class ForestPredictor(_PackedForest):
    """A packed forest on one device. Build with :meth:`from_sklearn`.

    ``nodes`` is the chunked kernel's 16-byte packing, or None when a tree
    exceeds its 2,048 nodes; ``split_nodes`` / ``leaf_values`` are the split
    walk's packing, which every forest has."""

    def __init__(self, nodes, tree_first, baseline, n_features, split_nodes, leaf_values,
                 classes=None, identity_link=True, device=None):
        super().__init__(nodes, tree_first, n_features, len(baseline), classes, device)
        self.rows_per_wg = rows_per_wg(self.n_features, self.n_scores)
        self.split_rows_per_wg = split_rows_per_wg(self.n_features)
        self.identity_link = bool(identity_link)
        self._baseline_np, self._baseline = baseline, self._upload(baseline)
        self._split_nodes_np, self._split_nodes = split_nodes, self._upload_nodes(split_nodes)
        self._leaf_values_np, self._leaf_values = leaf_values, self._upload(leaf_values)
        self._leaf_rows = None      # the split walk's scratch, grown on demand

    @classmethod
    def from_sklearn(cls, est, device=None):
        predictors = est._predictors
        K, F = len(predictors[0]), int(est.n_features_in_)
        trees = [tree.nodes for iteration in predictors for tree in iteration]
        cls._refuse_beyond_limits(K, "trees per iteration", F, sum(len(t) for t in trees))
        if any(t["is_categorical"].any() for t in trees):
            raise ValueError("categorical splits are not supported by the forest kernel")
        largest = max(len(t) for t in trees)
        if largest > SPLIT_MAX_TREE_NODES:
            raise ValueError(f"a tree has {largest} nodes: a child distance has 20 bits")
        # the 16-byte packing needs every tree in one LDS chunk
        nodes = (np.concatenate([_pack_tree(t) for t in trees]) if largest <= CHUNK_NODES
                 else None)
        packed, first_leaf_row = [], 0
        for t in trees:
            packed.append(_pack_split_tree(t, first_leaf_row))
            first_leaf_row += len(packed[-1][1])
        tree_first = np.concatenate([[0], np.cumsum([len(t) for t in trees])]).astype(np.int32)
        # sklearn starts from zeros + baseline
        baseline = 0.0 + np.asarray(est._baseline_prediction, dtype=np.float64).reshape(-1)
        assert len(baseline) == K
        return cls(nodes, tree_first, baseline, F, np.concatenate([p[0] for p in packed]),
                   np.concatenate([p[1] for p in packed]),
                   classes=getattr(est, "classes_", None),
                   identity_link=type(est._loss.link).__name__ == "IdentityLink",
                   device=device)

    # -- scoring ----------------------------------------------------------------

    def walk_for(self, n_rows, trees_per_chunk=0):
        """The path a call of ``n_rows`` rows takes when none is forced:
        "split" for a forest without the 16-byte packing, "chunked" under a
        ``trees_per_chunk`` cap, otherwise "split" up to ``split_max_rows``."""
        if self._nodes_np is None:
            return "split"
        if trees_per_chunk > 0:
            return "chunked"
        return "split" if n_rows <= split_max_rows else "chunked"

    def _score(self, X, trees_per_chunk=0, walk=None, prefix_nodes=-1, trees_per_slice=0):
        """-> (scores fp64 [B][K], class indices int32 [B]) on the device."""
        if walk is None:
            walk = self.walk_for(X.shape[0] if hasattr(X, "shape") else len(X), trees_per_chunk)
        if walk not in ("chunked", "split"):
            raise ValueError(f'walk must be "chunked", "split" or None, is {walk!r}')
        if walk == "chunked" and self._nodes_np is None:
            raise ValueError(f"a tree has {self.max_tree_nodes} nodes: the chunked kernel "
                             f"takes {CHUNK_NODES}, only the split walk serves this forest")
        return self._run(X, walk, trees_per_chunk, prefix_nodes, trees_per_slice)

    def _launch(self, X, scores, labels, walk, trees_per_chunk, prefix_nodes, trees_per_slice):
        if walk == "chunked":
            self._ext.forest_predict(X, self._nodes, self._first, self._baseline,
                                     self.max_tree_nodes, scores, labels, trees_per_chunk)
            return
        # leaf_rows [T][rows] of one launch stays within SPLIT_SCRATCH_BYTES:
        # rows are independent, so row blocks give the same bits
        B, T = X.shape[0], self.n_trees
        block = min(B, max(1, SPLIT_SCRATCH_BYTES // (4 * T)))
        if self._leaf_rows is None or self._leaf_rows.numel() < T * block:
            self._leaf_rows = torch.empty(T * block, dtype=torch.int32, device=self.device)
        for b0 in range(0, B, block):
            b1 = min(B, b0 + block)
            self._ext.forest_split_predict(
                X[b0:b1], self._split_nodes, self._first, self._leaf_values, self._baseline,
                self.max_tree_nodes, self._leaf_rows, scores[b0:b1], labels[b0:b1],
                prefix_nodes, trees_per_slice)

    def _host(self, X, walk, *caps):
        s = self._walk_cpu(X)[0] if walk == "chunked" else self._walk_split_cpu(X)
        return s, (s[:, 0] > 0) if self.n_scores == 1 else s.argmax(axis=1)   # first largest

    def _walk_split_cpu(self, X):
        """The split packing walked on the host, the trees' leaves added in
        the sum kernel's order -> scores fp64 [B][K]."""
        scores = np.tile(self._baseline_np, (X.shape[0], 1))
        for t in range(self.n_trees):
            leaves = _leaves_cpu(self._split_nodes_np, self._first_np, X, t)
            scores[:, t % self.n_scores] += self._leaf_values_np[leaves]
        return scores

    def _walk_cpu(self, X):
        """The 16-byte packing walked on the host, tree by tree in the chunked
        kernel's order -> (scores fp64 [B][K], node visits, leaves included)."""
        nodes, first, K = self._nodes_np, self._first_np, self.n_scores
        thr, meta, value = nodes["thr"], nodes["meta"], nodes["value"]
        B = X.shape[0]
        rows = np.arange(B)
        scores = np.tile(self._baseline_np, (B, 1))
        visits = 0
        for t in range(self.n_trees):
            base = int(first[t])
            idx = np.full(B, base)
            while True:
                m = meta[idx]
                x = X[rows, m & 0xFFFF]
                go_left = np.where(np.isnan(x), (m >> 31) != 0, x <= thr[idx])
                nxt = base + ((m >> META_LEFT_SHIFT) & 0x7FFF) + np.where(go_left, 0, 1)
                visits += int((nxt != idx).sum())
                if np.array_equal(nxt, idx):
                    break
                idx = nxt
            visits += B
            scores[:, t % K] += value[idx]
        return scores, visits

    def decision_function(self, X, trees_per_chunk=0, walk=None, prefix_nodes=-1,
                          trees_per_slice=0):
        """Raw scores, fp64 ``[B][K]`` on the predictor's device: sklearn's
        ``decision_function`` (``predict`` for an identity-link regressor) bit
        for bit. ``walk`` forces the "chunked" kernel or the "split" walk
        (None: :meth:`walk_for`). ``trees_per_chunk`` caps the chunked
        kernel's trees per LDS chunk, ``prefix_nodes`` and ``trees_per_slice``
        the split walk's LDS prefix and slice (tests)."""
        return self._score(X, trees_per_chunk, walk, prefix_nodes, trees_per_slice)[0]

    def predict(self, X, trees_per_chunk=0, walk=None, prefix_nodes=-1, trees_per_slice=0):
        """Classifier: labels by the raw-score argmax (ties to the lowest
        class; ``score > 0`` when binary) through ``classes_``, a numpy array.
        Regressor: the values, fp64 ``[B]`` on the device."""
        if self.classes_ is None and not self.identity_link:
            raise ValueError("predict() of a regressor with a non-identity link is not "
                             "supported; decision_function() returns the raw scores")
        scores, labels = self._score(X, trees_per_chunk, walk, prefix_nodes, trees_per_slice)
        if self.classes_ is None:
            return scores[:, 0]
        return self.classes_[labels.cpu().numpy()]

    def predict_proba(self, X, walk=None):
        """softmax (sigmoid when binary) of the raw scores, with torch on the
        device; fp64 ``[B][n_classes]``."""
        if self.classes_ is None:
            raise ValueError("predict_proba() needs a classifier")
        s = self.decision_function(X, walk=walk)
        if self.n_scores == 1:
            p = torch.sigmoid(s)
            return torch.cat([1.0 - p, p], dim=1)
        return torch.softmax(s, dim=1)


# ---------------------------------------------------------------------------
# bagged forests: random forests, extra-trees, single decision trees
# ---------------------------------------------------------------------------

# the Python copy of hip/bagged_forest.h (a GPU test holds the two equal)
BAGGED_MAX_TREE_NODES = 1 << 20
BAGGED_MIN_ROWS, BAGGED_MAX_ROWS = 4, 256
BAGGED_MAX_ITEMS = 2048         # rows x values a leaf of one workgroup
BAGGED_WALK_ITEMS = 2048        # rows x trees of one chunk
BAGGED_CHUNK_TREES = 256
BAGGED_TILE_BYTES = 80 * 1024 - (2048 * 8 + BAGGED_MAX_ITEMS * 8 + BAGGED_WALK_ITEMS * 4
                                 + 2 * 2 * BAGGED_CHUNK_TREES * 4)

# a leaf's "thr" holds its leaf_values row, so both fields are kept as bits
BAGGED_NODE_DTYPE = np.dtype([("thr", "<u4"), ("meta", "<u4")])
BAGGED_META_MISSING_LEFT, BAGGED_META_DIST_SHIFT = 1 << 11, 12


def bagged_rows_per_wg(n_features: int, n_scores: int) -> int:
    """Rows per workgroup of the bagged kernel: up to 256, rows x values
    within 2,048 sums."""
    return _tile_rows(n_features, n_scores, BAGGED_MAX_ROWS, BAGGED_TILE_BYTES,
                      BAGGED_MAX_ITEMS)


def bagged_trees_per_chunk(rows: int, n_trees: int, cap: int = 0) -> int:
    """Trees a workgroup that holds ``rows`` rows walks at once."""
    rp = 1
    while rp < rows:
        rp *= 2
    n = min(BAGGED_WALK_ITEMS // rp, BAGGED_CHUNK_TREES, n_trees)
    return min(n, cap) if cap > 0 else n


def _pack_bagged_tree(tree, first_leaf_row):
    """One sklearn ``Tree`` -> (packed nodes, leaf values [leaves][K]),
    renumbered breadth-first; leaves number the rows of leaf_values from
    ``first_leaf_row`` in that order."""
    left, right = tree.children_left, tree.children_right
    order, new_of = _breadth_first(left, right, left >= 0)
    n = len(order)
    leaf = left[order] < 0
    dist = np.where(leaf, 0, new_of[np.where(leaf, 0, left[order])] - np.arange(n))
    assert np.all(leaf | (new_of[right[order]] == np.arange(n) + dist + 1))
    assert dist.max(initial=0) < BAGGED_MAX_TREE_NODES
    missing = getattr(tree, "missing_go_to_left", None)
    missing_left = np.zeros(n, bool) if missing is None else missing[order].astype(bool)
    out = np.zeros(n, dtype=BAGGED_NODE_DTYPE)
    out["thr"] = np.where(leaf, first_leaf_row + np.cumsum(leaf) - 1,
                          rd32(tree.threshold[order]).view(np.uint32))
    out["meta"] = (np.where(leaf, 0, tree.feature[order]).astype(np.uint32)
                   | np.where(~leaf & missing_left, np.uint32(BAGGED_META_MISSING_LEFT),
                              np.uint32(0))
                   | (dist.astype(np.uint32) << BAGGED_META_DIST_SHIFT))
    return out, np.ascontiguousarray(tree.value[order[leaf], 0, :], dtype=np.float64)


def _is_bagged(est) -> bool:
    from sklearn import ensemble, tree

    # ExtraTreeClassifier / ExtraTreeRegressor derive from the DecisionTree classes
    return isinstance(est, (ensemble.RandomForestClassifier, ensemble.RandomForestRegressor,
                            ensemble.ExtraTreesClassifier, ensemble.ExtraTreesRegressor,
                            tree.DecisionTreeClassifier, tree.DecisionTreeRegressor))


class BaggedForestPredictor(_PackedForest):
    """A packed random forest, extra-trees ensemble or single decision tree
    on one device: the mean over the trees of the leaves' fp64 vectors, in
    sklearn's ``n_jobs=None`` order, bit for bit (docs/kernels.md
    "Bagged-forest inference"). Build with :meth:`from_sklearn`."""

    def __init__(self, nodes, tree_first, leaf_values, n_features, classes=None, device=None):
        super().__init__(nodes, tree_first, n_features, leaf_values.shape[1], classes, device)
        self.rows_per_wg = bagged_rows_per_wg(self.n_features, self.n_scores)
        self._values_np, self._values = leaf_values, self._upload(leaf_values)

    @classmethod
    def from_sklearn(cls, est, device=None):
        if not _is_bagged(est):
            raise TypeError(f"{type(est).__name__} is no random forest, extra-trees "
                            "ensemble or decision tree")
        trees = [e.tree_ for e in getattr(est, "estimators_", [est])]
        if int(est.n_outputs_) > 1:
            raise ValueError(f"{est.n_outputs_} outputs: the bagged kernel takes one")
        classes = getattr(est, "classes_", None)
        K, F = 1 if classes is None else len(classes), int(est.n_features_in_)
        cls._refuse_beyond_limits(K, "classes", F, sum(t.node_count for t in trees))
        largest = max(t.node_count for t in trees)
        if largest > BAGGED_MAX_TREE_NODES:
            raise ValueError(f"a tree has {largest} nodes: a child distance has 20 bits")
        packed, first_leaf_row = [], 0
        for t in trees:
            packed.append(_pack_bagged_tree(t, first_leaf_row))
            first_leaf_row += len(packed[-1][1])
        nodes = np.concatenate([p[0] for p in packed])
        leaf_values = np.concatenate([p[1] for p in packed])
        tree_first = np.concatenate([[0], np.cumsum([t.node_count for t in trees])])
        return cls(nodes, tree_first.astype(np.int32), leaf_values, F, classes=classes,
                   device=device)

    # -- scoring ----------------------------------------------------------------

    def _score(self, X, prefix_nodes=-1, trees_per_chunk=0):
        """-> (means fp64 [B][K], class indices int32 [B]) on the device."""
        return self._run(X, prefix_nodes, trees_per_chunk)

    def _launch(self, X, probs, labels, prefix_nodes, trees_per_chunk):
        self._ext.bagged_forest_predict(X, self._nodes, self._first, self._values,
                                        self.max_tree_nodes, probs, labels, prefix_nodes,
                                        trees_per_chunk)

    def _host(self, X, *caps):
        p = self._walk_cpu(X)
        return p, p.argmax(axis=1)   # first largest

    def _leaves_cpu(self, X, t):
        """leaf_values rows that the rows of X reach in tree t."""
        return _leaves_cpu(self._nodes_np, self._first_np, X, t)

    def _walk_cpu(self, X):
        """The packed arrays walked on the host, the trees added in order and
        the sum divided once, as the kernel does -> fp64 [B][K]."""
        acc = np.zeros((X.shape[0], self.n_scores))
        for t in range(self.n_trees):
            acc += self._values_np[self._leaves_cpu(X, t)]
        acc /= self.n_trees
        return acc

    def predict_proba(self, X, prefix_nodes=-1, trees_per_chunk=0):
        """Class probabilities, fp64 ``[B][n_classes]`` on the predictor's
        device: sklearn's ``predict_proba`` (fitted with ``n_jobs=None``) bit
        for bit. ``prefix_nodes`` and ``trees_per_chunk`` cap the kernel's
        LDS prefix and chunk (tests)."""
        if self.classes_ is None:
            raise ValueError("predict_proba() needs a classifier")
        return self._score(X, prefix_nodes, trees_per_chunk)[0]

    def predict(self, X, prefix_nodes=-1, trees_per_chunk=0):
        """Classifier: ``classes_`` at the first largest probability, a numpy
        array. Regressor: the values, fp64 ``[B]`` on the device."""
        probs, labels = self._score(X, prefix_nodes, trees_per_chunk)
        if self.classes_ is None:
            return probs[:, 0]
        return self.classes_[labels.cpu().numpy()]


def from_sklearn(est, device=None):
    """The device predictor of a fitted sklearn tree model: a
    :class:`ForestPredictor` for ``HistGradientBoosting*``, a
    :class:`BaggedForestPredictor` for ``RandomForest*``, ``ExtraTrees*``,
    ``DecisionTree*`` and ``ExtraTree*``."""
    if hasattr(est, "_predictors"):
        return ForestPredictor.from_sklearn(est, device=device)
    if _is_bagged(est):
        return BaggedForestPredictor.from_sklearn(est, device=device)
    raise TypeError(f"no device predictor for {type(est).__name__}")


class _ForestCache:
    """The packed forest of a fitted estimator, kept on the estimator object.
    Valid while the estimator holds the same list of trees (``_predictors``
    of a boosted estimator, ``estimators_`` of a bagged one) at the same
    length: a refit makes a new list, a warm start extends it. Pickles as an
    empty cache, so that a saved artifact holds no device memory."""

    def __init__(self):
        self.trees, self.count, self.forest = None, 0, None

    def __reduce__(self):
        return (_ForestCache, ())

    def get(self, est):
        trees = est._predictors if hasattr(est, "_predictors") else est.estimators_
        if self.trees is not trees or self.count != len(trees):
            self.forest = from_sklearn(est)
            self.trees, self.count = trees, len(trees)
        return self.forest


def device_forest(est):
    """The device predictor of a fitted boosted or bagged ensemble, built
    once per fit and kept on the estimator."""
    cache = getattr(est, "_unionml_forest", None)
    if cache is None:
        cache = est._unionml_forest = _ForestCache()
    return cache.get(est)
