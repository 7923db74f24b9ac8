"""Host-side tests of the evaluation candidates (``data/candidates.py``, ``training/catalogue.py``) and of the numpy
restatement the GPU tests compare against (``tests/candidates_reference.py``): the integer weights, every refusal
with its message, the new entry points, and the distribution of the restated weighted draw."""
import numpy as np
import pytest

from tests import candidates_reference as CR
from tests.test_cpu_device_epoch import _dataset

W1 = 1 << 24


# ----------------------------------------------------------------------------- item_weights
def test_item_weights_range_monotone_and_zero_count():
    from deepfm_amd.data import item_weights
    counts = np.array([0, 1, 2, 3, 10, 10, 500, 100000, 7])
    for alpha in (0.25, 0.75, 1.0, 2.0):
        w = item_weights(counts, alpha)
        assert w.dtype == np.uint32 and w.shape == counts.shape
        assert w.min() >= 1 and w.max() == W1
        order = np.argsort(counts, kind="stable")
        assert (np.diff(w[order].astype(np.int64)) >= 0).all(), "not monotone in the count"
        assert w[0] == w[1], "a zero count counts as 1"
        assert w[4] == w[5]
    assert item_weights(counts, 1.0)[6] == round(500 / 100000 * W1)
    assert item_weights(np.array([1, 10 ** 9]), 2.0)[0] == 1          # clamped below at 1


def test_item_weights_alpha_zero_is_uniform_and_bad_input_is_refused():
    from deepfm_amd.data import item_weights
    assert (item_weights([0, 5, 90], 0.0) == W1).all()
    for bad in ([], [1, -1], [1, np.nan]):
        with pytest.raises(ValueError, match="item_weights: counts"):
            item_weights(bad, 0.75)


# ----------------------------------------------------------------------------- the library
def test_library_exports_the_candidate_symbols():
    from deepfm_amd import _lib
    lib = _lib.load()
    for name in ("dfm_sample_weighted", "dfm_catalogue_topk"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    assert _lib.MAX_NEGATIVES == 16 and _lib.MAX_CANDIDATES == 1 << 20 and _lib.WEIGHTED_MAX_ITEMS >= 65536


# ----------------------------------------------------------------------------- refusals
def _source(cls, **kw):
    import torch
    from deepfm_amd.data import DeviceColumns, ItemTable, SeenSets
    schema, cols, user_of, items = _dataset()
    n_users, n_items = 5, 40
    args = dict(columns=DeviceColumns(cols, torch.device("cpu")),
                seen=SeenSets.from_interactions(user_of, cols.ids[1] - 1, n_users, n_items), user_of=user_of,
                items=ItemTable(schema, items))
    if cls.__name__ == "WeightedNegatives":
        args.update(weights=np.arange(1, n_items + 1, dtype=np.uint32), num_neg=20)
    for k, v in kw.items():
        args[k] = v(args, cols, user_of) if callable(v) else v
    return cls(**args)


def test_valid_sources_build_on_the_host():
    from deepfm_amd.data import CatalogueCandidates, Role, WeightedNegatives
    w = _source(WeightedNegatives)
    assert w.neg_items.shape == (30, 20) and w.num_neg == 20
    c = _source(CatalogueCandidates)
    assert c.num_neg == 40 and (c.neg_items.numpy() == np.arange(40)[None, :]).all()
    for s in (w, c):
        assert {k for k, r in s.roles.items() if r is Role.ITEM} == {"movie_id", "genres", "item_count"}


@pytest.mark.parametrize("weights, msg", [
    (np.arange(1, 40, dtype=np.uint32), r"weights has shape \(39,\) for 40 item rows"),
    (np.zeros(40, np.uint32), r"weights must be integers in \[1, 16777216\]"),
    (np.full(40, W1 + 1, np.uint32), r"weights must be integers in \[1, 16777216\]"),
    (np.ones(40, np.float32), r"weights must be integers in \[1, 16777216\]"),
])
def test_refuses_weights_out_of_range_or_of_the_wrong_length(weights, msg):
    from deepfm_amd.data import WeightedNegatives
    with pytest.raises(ValueError, match=msg):
        _source(WeightedNegatives, weights=weights)


def test_refuses_user_with_fewer_unseen_rows_than_num_neg():
    from deepfm_amd.data import SeenSets, WeightedNegatives

    def seen(a, cols, user_of):
        victim = int(user_of[0])
        return SeenSets.from_interactions(list(user_of) + [victim] * 38, list(cols.ids[1] - 1) + list(range(38)), 5, 40)

    _, _, user_of, _ = _dataset()
    with pytest.raises(ValueError, match=rf"user {int(user_of[0])} has [012] unseen items, fewer than num_neg = 20"):
        _source(WeightedNegatives, seen=seen)
    with pytest.raises(ValueError, match=r"num_neg = 0 outside \[1, 1048576\]"):
        _source(WeightedNegatives, num_neg=0)
    from deepfm_amd.data import CatalogueCandidates
    _source(CatalogueCandidates, seen=seen)              # the catalogue needs no unseen row at all


def test_sources_share_the_role_rules():
    from deepfm_amd.data import CatalogueCandidates, Role, WeightedNegatives
    for cls in (WeightedNegatives, CatalogueCandidates):
        with pytest.raises(ValueError, match="'gender' has role ITEM but the item table has no column"):
            _source(cls, roles={"gender": Role.ITEM})
        with pytest.raises(ValueError, match="user_of names a user outside the seen-sets"):
            _source(cls, user_of=lambda a, cols, u: np.where(np.arange(u.size) == 3, 5, u))


def test_refuses_a_score_matrix_over_the_cap(monkeypatch):
    from deepfm_amd.data import CatalogueCandidates, candidates
    assert candidates.CATALOGUE_MAX_BYTES == 1 << 30
    monkeypatch.setattr(candidates, "CATALOGUE_MAX_BYTES", 4 * 30 * 40 - 1)
    with pytest.raises(ValueError, match=r"score matrix of 30 queries x 40 items takes 4800 bytes, more than 4799"):
        _source(CatalogueCandidates)
    monkeypatch.setattr(candidates, "CATALOGUE_MAX_BYTES", 4 * 30 * 40)
    _source(CatalogueCandidates)


def test_refuses_a_loader_built_over_other_columns():
    import torch
    from deepfm_amd.data import CatalogueCandidates, DeviceColumns, DeviceEpochLoader, WeightedNegatives
    _, cols, _, _ = _dataset()
    other = DeviceColumns(cols, torch.device("cpu"))
    for cls in (WeightedNegatives, CatalogueCandidates):
        with pytest.raises(ValueError, match="built over other columns"):
            DeviceEpochLoader(other, 8, negatives=_source(cls))


class _Predictor:
    """What ``CatalogueScorer`` checks before it touches the device."""
    B = 8

    def __init__(self, schema):
        self.model = type("M", (), {"schema": schema})()


def test_scorer_refuses_k_outside_1_to_128_and_another_schema(monkeypatch):
    import torch
    from deepfm_amd.data import CatalogueCandidates, DeviceEpochLoader
    from deepfm_amd.training import CatalogueScorer
    monkeypatch.setattr(DeviceEpochLoader, "__init__", lambda self, *a, **k: None)   # its plan needs the device
    monkeypatch.setattr(DeviceEpochLoader, "__del__", lambda self: None)
    cand = _source(CatalogueCandidates)
    scorer = CatalogueScorer(_Predictor(cand.columns.schema), cand)
    scores = torch.zeros(30, 40)
    for k in (0, 129, -3):
        with pytest.raises(ValueError, match=rf"k = {k} outside \[1, 128\]"):
            scorer._topk(scores, None, k, True)
    scorer.predictor.device = torch.device("cpu")
    with pytest.raises(ValueError, match="every k must be at most 128"):
        scorer.evaluate(np.zeros(30, np.int32), ks=[10, 129])
    from tests.test_cpu_device_epoch import _schema
    fields = dict(_schema().fields)
    fields.pop("gender")
    with pytest.raises(ValueError, match="candidates of another schema"):
        CatalogueScorer(_Predictor(type(cand.columns.schema)(fields=fields)), cand)


# ----------------------------------------------------------------------------- the restated draw
def test_restated_weighted_draw_follows_the_weights():
    """One user with 8 unseen rows of weights 1 .. 2^24, 200 000 draws: every row's frequency within 5 standard
    deviations sqrt(n p (1 - p)) of n w_i / T.  Fixed seed: deterministic."""
    n_items, n = 12, 200_000
    rows = np.array([0, 2, 3, 5, 7, 8, 10, 11])
    weights = np.full(n_items, 12345, np.uint32)
    weights[rows] = [1, 1 << 4, 1 << 12, 1 << 20, 3 << 21, 1 << 23, 12_000_000, W1]
    got = CR.weighted_draws(rows, weights, p=0, C=n, seed=7, epoch=0)
    assert set(got.tolist()) <= set(rows.tolist())
    T = float(weights[rows].astype(np.uint64).sum())
    for i in rows:
        p = float(weights[i]) / T
        cnt, sd = int((got == i).sum()), np.sqrt(n * p * (1 - p))
        print(f"row {i}: weight {int(weights[i])}, {cnt} draws, expected {n * p:.2f} +- {sd:.2f}")
        assert abs(cnt - n * p) <= 5 * sd
    again = CR.weighted_draws(rows, weights, p=0, C=n, seed=7, epoch=0)
    assert np.array_equal(got, again)
    assert not np.array_equal(got, CR.weighted_draws(rows, weights, p=0, C=n, seed=7, epoch=1))
    assert not np.array_equal(got[:1000], CR.weighted_draws(rows, weights, p=1, C=1000, seed=7, epoch=0))


def test_restated_draw_edges_and_selection_order():
    w = np.array([5, 1, W1, 9], np.uint32)
    assert (CR.weighted_draws(np.array([2]), w, 3, 50, 1, 0) == 2).all()          # one unseen row: always that row
    assert (CR.weighted_draws(np.zeros(0, np.int64), w, 3, 5, 1, 0) == -1).all()
    s = np.array([[0.5, -0.0, 0.0, 0.5, np.inf, -np.inf, 0.25]], np.float32)
    items, top, rank, status = CR.catalogue_topk(s, [{4}], [0], [6], 4, True, 1)
    assert items.tolist() == [[0, 3, 6, 1]] and rank.tolist() == [2] and status == [0, 0, 0]
    assert np.array_equal(top.view(np.uint32), s[0, [0, 3, 6, 1]].view(np.uint32)[None])
    items, _, rank, status = CR.catalogue_topk(s, [set(range(7))], [0], [4], 3, True, 1)
    assert items.tolist() == [[4, -1, -1]] and rank.tolist() == [0]               # seen everything: the target only
    assert CR.catalogue_topk(s, [set()], [1], [7], 1, True, 1)[3] == [0, 1, 1]
    m = CR.full_ranking_metrics(np.array([0, 3, -1, 12]), [1, 5])
    assert m["HR@1"] == 1 / 3 and m["HR@5"] == 2 / 3 and m["NDCG@1"] == 1 / 3
