"""forest_predict_kernel against sklearn's own fp64 scores, bit for bit: every
model of forest_fixtures at B = 1, R - 1, R + 1, 2R + 17 under three
chunkings, the binding's preconditions, and the boosting app."""

import numpy as np
import pytest
import torch
from forest_fixtures import MODELS, fitted, probe_rows, raw_argmax_labels, sklearn_scores

from unionml_amd.ops import forest as F

pytestmark = pytest.mark.gpu
POISON_SCORE, POISON_LABEL = -7.25, -5
UNEVEN = 5   # trees per chunk: divides no tree count here, a multiple of no K > 1


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
            X = probe_rows(forest, 2 * forest.rows_per_wg + 17)
            out[name] = (est, forest, torch.from_numpy(X).cuda(), sklearn_scores(est, X))
        return out[name]

    return get


def launch(ext, forest, X, B, trees_per_chunk, spare=3):
    scores = torch.full((B + spare, forest.n_scores), POISON_SCORE, dtype=torch.float64,
                        device="cuda")
    labels = torch.full((B + spare,), POISON_LABEL, dtype=torch.int32, device="cuda")
    ext.forest_predict(X[:B], forest._nodes, forest._first, forest._baseline,
                       forest.max_tree_nodes, scores, labels, trees_per_chunk)
    return scores, labels


@pytest.mark.parametrize("trees_per_chunk", [0, 1, UNEVEN])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_kernel_equals_sklearn_bit_for_bit(ext, cases, name, trees_per_chunk):
    est, forest, X, want = cases(name)
    R, K, T = forest.rows_per_wg, forest.n_scores, forest.n_trees
    assert R == ext.forest_rows_per_wg(forest.n_features, K)
    assert T % UNEVEN != 0 and (K == 1 or UNEVEN % K != 0)
    for B in (1, R - 1, R + 1, 2 * R + 17):
        scores, labels = launch(ext, forest, X, B, trees_per_chunk)
        ref = torch.from_numpy(want[:B]).cuda()
        assert torch.equal(scores[:B], ref), (name, B)
        idx = (ref[:, 0] > 0).int() if K == 1 else ref.argmax(dim=1).int()
        assert torch.equal(labels[:B], idx), (name, B)
        assert bool((scores[B:] == POISON_SCORE).all()) and bool((labels[B:] == POISON_LABEL).all())
        again = launch(ext, forest, X, B, trees_per_chunk)
        assert torch.equal(again[0], scores) and torch.equal(again[1], labels)
    if hasattr(est, "classes_"):
        assert np.array_equal(forest.predict(X), raw_argmax_labels(est, want))


def test_constants_match_the_header(ext):
    assert (ext.FOREST_CHUNK_NODES, ext.FOREST_CHUNK_TREES, ext.FOREST_MAX_FEATURES) == (
        F.CHUNK_NODES, F.CHUNK_TREES, F.MAX_FEATURES)


@pytest.mark.parametrize("broken", ["dtype", "k_width", "short_labels", "strided_x",
                                    "aliased", "k_zero"])
def test_binding_preconditions(ext, cases, broken):
    _, forest, X, _ = cases("classes3")
    B, K = 40, forest.n_scores
    args = dict(X=X[:B].clone(), baseline=forest._baseline,
                scores=torch.full((B, K), POISON_SCORE, dtype=torch.float64, device="cuda"),
                labels=torch.full((B,), POISON_LABEL, dtype=torch.int32, device="cuda"))
    if broken == "dtype":
        args["X"] = args["X"].double()
    elif broken == "k_width":
        args["scores"] = torch.full((B, K + 1), POISON_SCORE, dtype=torch.float64, device="cuda")
    elif broken == "short_labels":
        args["labels"] = args["labels"][: B - 1]
    elif broken == "strided_x":
        args["X"] = torch.cat([args["X"], args["X"]], dim=1)[:, ::2]
    elif broken == "aliased":
        args["labels"] = args["X"].view(torch.int32).view(-1)[:B]
    elif broken == "k_zero":
        args["baseline"] = forest._baseline[:0]
        args["scores"] = args["scores"][:, :0]
    kept = {k: v.clone().contiguous() for k, v in args.items()}
    with pytest.raises(RuntimeError):
        ext.forest_predict(args["X"], forest._nodes, forest._first, args["baseline"],
                           forest.max_tree_nodes, args["scores"], args["labels"])
    torch.cuda.synchronize()
    assert all(torch.equal(v.contiguous().view(torch.uint8), kept[k].view(torch.uint8))
               for k, v in args.items())


def test_boosting_app_predicts_on_the_device():
    from unionml_amd.models import gbdt

    gbdt.model.artifact = None
    clf, _ = gbdt.model.train(trainer_kwargs={"max_iter": 20}, n=400)
    frame = gbdt.reader(n=400)[gbdt.FEATURES]
    got = gbdt.predictor(clf, frame)
    assert gbdt.device_forest(clf) is gbdt.device_forest(clf)
    raw = clf.decision_function(frame)
    assert got == [int(c) for c in clf.classes_[raw.argmax(axis=1)]]
