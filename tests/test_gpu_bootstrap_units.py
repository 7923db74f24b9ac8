"""GPU: the bootstrap of the per-user metrics (csrc/bootstrap_units.hip and the per-user columns of csrc/ranking.hip and
csrc/grouped_auc.hip) against the numpy restatement (tests/bootstrap_units_reference.py), bit for bit unless said
otherwise: the wrapping column sums at the edges of the wave, the chunk, the replicate block and the column templates;
the weights against the pooled bootstrap's; the per-user ranks and group columns; ``compute_bootstrap_ranking`` /
``compare_bootstrap_ranking``; the predictors and the Trainer."""
import json

import numpy as np
import pytest
import torch

from tests import bootstrap_reference as BR
from tests import bootstrap_units_reference as UR
from tests.grouped_auc_reference import group_integers

pytestmark = pytest.mark.gpu

# 2^-30 is the unit of the gains and of auc_g: a rounding moves a term by at most 2^-31, and so a mean of terms
RESOLUTION = 1e-9
SPREAD = ("se", "lo", "hi", "replicates")


def _chunk():
    from deepfm_amd import _lib
    return _lib.BOOTSTRAP_UNITS_CHUNK


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))      # == on the doubles


def _same_dict(got, want):
    assert list(got) == list(want), (list(got), list(want))
    bad = [k for k in got if not (got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])))]
    assert not bad, [(k, got[k], want[k]) for k in bad]


def _spread_keys(names):
    return [f"{m}_{k}" for m in names for k in SPREAD]


# ----------------------------------------------------------------------------- dfm_bootstrap_units
def _units_sums(cols_u64, replicates, seed, misalign):
    """The device sums of (num_cols, num_units) uint64 columns; ``misalign``: the base is 8 bytes past a 16-byte line."""
    from deepfm_amd.training import bootstrap_units_device
    C, U = cols_u64.shape
    buf = torch.empty(C * U + 1, dtype=torch.int64, device="cuda")
    view = buf[1:] if misalign else buf[:-1]
    view.copy_(_dev(cols_u64.view(np.int64).reshape(-1)))
    cols = view.view(C, U)
    assert cols.data_ptr() % 16 == (8 if misalign else 0)
    sums = bootstrap_units_device(cols, replicates, seed)
    assert sums.shape == (replicates, C) and sums.dtype == torch.int64
    return sums.cpu().numpy().view(np.uint64)


def _sizes():
    C = _chunk()
    return [1, 2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7]


@pytest.mark.parametrize("k", range(9))
def test_wrapping_sums_match_numpy(k):
    """Every num_units at an edge of the wave and of the chunk, crossed with the replicates around a replicate block,
    a column count of every kernel template, both alignments of the base and two seeds; full-range uint64 columns."""
    U = _sizes()[k]
    rng = np.random.default_rng(200 + k)
    for C in (1, 2, 17, 24):
        cols = rng.integers(0, 1 << 64, (C, U), dtype=np.uint64)
        for R in (1, 15, 16, 17, 33):
            for misalign, seed in ((False, 0), (True, 0x9E3779B97F4A7C15)):
                got = _units_sums(cols, R, seed, misalign)
                want = UR.weighted_sums(cols, R, seed)
                assert np.array_equal(got, want), f"units {U} cols {C} R {R} misaligned {misalign}"


@pytest.mark.parametrize("C", [4, 5, 8, 9, 13, 16])
def test_every_column_count_at_a_template_edge(C):
    U, R = _chunk() + 77, 17
    cols = np.random.default_rng(C).integers(0, 1 << 64, (C, U), dtype=np.uint64)
    assert np.array_equal(_units_sums(cols, R, 3, False), UR.weighted_sums(cols, R, 3))


def test_more_chunks_than_slabs_and_one_seed_one_result():
    """40 chunks share 16 copies of the sums; the same call twice is identical, another seed is not."""
    U, R, C = 40 * _chunk() + 5, 18, 9
    cols = np.random.default_rng(1).integers(0, 1 << 40, (C, U), dtype=np.uint64)
    a, b, other = _units_sums(cols, R, 5, False), _units_sums(cols, R, 5, False), _units_sums(cols, R, 6, False)
    assert np.array_equal(a, b) and not np.array_equal(a, other)
    assert np.array_equal(a, UR.weighted_sums(cols, R, 5))


def test_the_weights_are_the_pooled_bootstraps():
    """sum_u w_u count_u over the bincount column is column S of the pooled bootstrap resampled by user, on the device."""
    from deepfm_amd.training import bootstrap_device, bootstrap_units_device
    rng = np.random.default_rng(2)
    n, U, R = 5000, 1500, 33
    u = rng.integers(0, U, n)
    y = (rng.random(n) < 0.4).astype(np.float32)
    s = rng.random(n).astype(np.float32)
    counts = _dev(np.bincount(u, minlength=U)[None, :].astype(np.int64))
    for seed in (0, 77):
        pooled = bootstrap_device(_dev(y), _dev(s), R, seed, _dev(u))[0][:, 4]
        assert torch.equal(bootstrap_units_device(counts, R, seed)[:, 0], pooled)
    assert not torch.equal(bootstrap_units_device(counts, R, 1)[:, 0], pooled)


def test_units_wrapper_refuses_what_the_kernel_does_not_take():
    from deepfm_amd.training import bootstrap_units_device
    cols = torch.zeros(2, 10, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="replicates = 0"):
        bootstrap_units_device(cols, 0)
    with pytest.raises(ValueError, match="25 columns"):
        bootstrap_units_device(torch.zeros(25, 10, dtype=torch.int64, device="cuda"), 5)
    with pytest.raises(TypeError):
        bootstrap_units_device(cols.to(torch.float64), 5)
    # a transposed view is made contiguous, not misread
    t = torch.arange(30, dtype=torch.int64, device="cuda").view(10, 3).t()
    want = UR.weighted_sums(t.cpu().numpy(), 4, 2)
    assert np.array_equal(bootstrap_units_device(t, 4, 2).cpu().numpy().view(np.uint64), want)


# ----------------------------------------------------------------------------- per-user columns
def _population(rng, users, cands, layout, ties=True):
    """``users`` ids with 1 .. ``cands`` samples each: rounded scores with -0 / +0 ties, user 5 with negatives only, user
    11 with positives only, user 3 with one sample and id 7 with none; ``layout``: contiguous or interleaved."""
    sizes = rng.integers(2, cands + 1, users)
    sizes[3], sizes[7] = 1, 0
    u = np.repeat(np.arange(users, dtype=np.int64), sizes)
    y = (rng.random(u.size) < 0.3).astype(np.float32)
    y[u == 5], y[u == 11] = 0.0, 1.0
    s = rng.standard_normal(u.size).astype(np.float32)
    if ties:
        s = np.round(s, 1).astype(np.float32)
        s[::7], s[3::7] = 0.0, -0.0
    if layout == "interleaved":
        p = rng.permutation(u.size)
        u, y, s = u[p], y[p], s[p]
    return u, y, s


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
@pytest.mark.parametrize("require_both", [True, False])
def test_user_ranks_match_the_restatement(layout, require_both):
    from deepfm_amd import _lib
    from deepfm_amd.training import ranking_metrics_device, ranking_user_ranks_device
    rng = np.random.default_rng(30 + require_both)
    U, ks = 300, [1, 3, 10]
    u, y, s = _population(rng, U, 40, layout)
    rank, out = ranking_user_ranks_device(_dev(u), _dev(y), _dev(s), U, require_both)
    rank, out = rank.cpu().numpy(), out.cpu().numpy()
    want, counted, faults = UR.user_ranks(u, y, s, U, require_both)
    assert np.array_equal(rank, want) and out.tolist() == [counted, 0, 0, 0]
    assert rank[7] == UR.NOT_COUNTED and (rank[3] == UR.NOT_COUNTED) == require_both      # no sample / one sample
    assert (rank[5], rank[11]) == ((UR.NOT_COUNTED, UR.NOT_COUNTED) if require_both else (UR.MISS, 0))
    # the hits and the counted users are ranking_metrics_device's; its NDCG to the fixed-point resolution
    m = ranking_metrics_device(_dev(u), _dev(y), _dev(s), ks, U, require_both).cpu().numpy()
    assert m[0] == counted
    gain = UR.gain_table(max(ks))
    for j, k in enumerate(ks):
        hit = (rank >= 0) & (rank < k)
        assert hit.sum() / counted == m[1 + j]                                                 # == on the doubles
        ndcg = float(gain[rank[hit]].sum()) * UR.UNIT / counted
        assert abs(ndcg - m[1 + len(ks) + j]) <= RESOLUTION
    # the columns of the ranks
    import ctypes as C
    lib = _lib.load()
    cols = torch.empty(1 + 2 * len(ks), U, dtype=torch.int64, device="cuda")
    d_rank, d_gain = _dev(rank), _dev(gain)                                 # held until the launch has run
    _lib.check(lib.dfm_bootstrap_rank_columns(d_rank.data_ptr(), U, (C.c_int32 * 3)(*ks), 3, d_gain.data_ptr(),
                                              gain.size, cols.data_ptr(), _lib.stream_handle()))
    assert np.array_equal(cols.cpu().numpy(), UR.rank_columns(want, ks))


def test_user_ranks_count_the_faulty_samples():
    from deepfm_amd.training import compute_bootstrap_ranking, ranking_user_ranks_device
    rng = np.random.default_rng(32)
    U = 50
    u, y, s = _population(rng, U, 20, "interleaved")
    u[[2, 40]] = [-1, U]
    rank, out = ranking_user_ranks_device(_dev(u), _dev(y), _dev(s), U)
    want, counted, faults = UR.user_ranks(u, y, s, U)                      # bad ids enter nothing: the ranks stand
    assert faults == [2, 0, 0] and out.cpu().tolist() == [counted, 2, 0, 0] and np.array_equal(rank.cpu().numpy(), want)
    with pytest.raises(ValueError, match=r"^2 user ids outside \[0, num_users\)$"):
        compute_bootstrap_ranking(u, y, _dev(s), [1], 5, num_users=U)
    u[[2, 40]] = [0, 1]
    s[[9, 10, 300]] = np.nan
    assert ranking_user_ranks_device(_dev(u), _dev(y), _dev(s), U)[1].cpu().tolist()[1:] == [0, 3, 0]
    with pytest.raises(ValueError, match=r"^Input contains NaN\.$"):
        compute_bootstrap_ranking(u, y, _dev(s), [1], 5, num_users=U, group_auc=True)
    s[[9, 10, 300]] = 0.5
    y[[4]] = 0.5
    assert ranking_user_ranks_device(_dev(u), _dev(y), _dev(s), U)[1].cpu().tolist()[1:] == [0, 0, 1]
    with pytest.raises(ValueError, match=r"^1 labels other than 0 and 1$"):
        compute_bootstrap_ranking(u, y, _dev(s), [], 5, num_users=U, group_auc=True)


@pytest.mark.parametrize("layout", ["contiguous", "interleaved"])
def test_group_columns_match_the_restatement(layout):
    from deepfm_amd import _lib
    from deepfm_amd.training import grouped_auc_device
    rng = np.random.default_rng(33)
    U = 300
    u, y, s = _population(rng, U, 40, layout)
    n = u.size
    lib = _lib.load()
    du, dy, ds = _dev(u), _dev(y), _dev(s)
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.dfm_grouped_auc_workspace_bytes(n, U), dtype=torch.uint8, device="cuda")
    _lib.check(lib.dfm_grouped_auc_prepare(du.data_ptr(), dy.data_ptr(), ds.data_ptr(), n, U, keys.data_ptr(),
                                           ws.data_ptr(), _lib.stream_handle()))
    ordered = torch.sort(keys).values
    cols = torch.empty(4, U, dtype=torch.int64, device="cuda")
    _lib.check(lib.dfm_grouped_auc_unit_columns(ordered.data_ptr(), n, U, ws.data_ptr(), cols.data_ptr(),
                                                _lib.stream_handle()))
    cols = cols.cpu().numpy()
    assert np.array_equal(cols, UR.group_columns(u, y, s, U))
    num, P, N, _ = group_integers(u, y, s, U)
    qual = (P > 0) & (N > 0)
    assert np.array_equal(cols[0], qual.astype(np.int64)) and np.array_equal(cols[2], np.where(qual, P + N, 0))
    assert cols[0, 5] == cols[0, 11] == cols[0, 7] == cols[0, 3] == 0
    per_group = grouped_auc_device(du, dy, ds, U, per_group=True)[1].cpu().numpy()
    assert np.array_equal(np.isnan(per_group), ~qual)
    assert np.array_equal(cols[1][qual], np.rint(per_group[qual] * 2.0 ** 30).astype(np.int64))
    assert np.array_equal(cols[3], cols[2] * cols[1])


# ----------------------------------------------------------------------------- compute / compare
def test_compute_bootstrap_ranking_is_the_points_and_the_spread_of_the_replicates():
    from deepfm_amd.training import (bootstrap_grouped_device, compute_bootstrap_ranking, compute_gauc,
                                     compute_ranking_metrics)
    rng = np.random.default_rng(40)
    U, R, ks = 1300, 70, [1, 5, 10, 20]                                     # two chunks of users
    u, y, s = _population(rng, U, 30, "interleaved")
    for group_auc, cut, level, seed in ((True, ks, 0.95, 2), (False, ks[:2], 0.8, 3), (True, [], 0.95, 4)):
        names = UR.names(cut, group_auc)
        values, faults = bootstrap_grouped_device(_dev(u), _dev(y), _dev(s), cut, R, seed, U, group_auc)
        want_values = UR.bootstrap_grouped(u, y, s, cut, R, seed, U, group_auc)
        assert values.dtype == torch.float64 and faults.cpu().tolist() == [0, 0, 0]
        assert _same(values.cpu().numpy(), want_values), (group_auc, cut)
        d = compute_bootstrap_ranking(u, y, _dev(s), cut, R, seed, U, group_auc, level)
        points = {**(compute_ranking_metrics(u, y, _dev(s), cut, U) if cut else {}),
                  **(compute_gauc(u, y, _dev(s), U) if group_auc else {})}
        assert list(d) == list(points) + _spread_keys(names) and {k: d[k] for k in points} == points
        _same_dict({k: d[k] for k in _spread_keys(names)}, UR.summary(want_values, names, level))
        for m in names:                        # (HR@20 of at most 30 candidates is 1 in most replicates)
            assert d[f"{m}_replicates"] == R and d[f"{m}_lo"] <= d[m] <= d[f"{m}_hi"] and d[f"{m}_se"] >= 0, m
        first = names[0]
        assert d[f"{first}_lo"] < d[first] < d[f"{first}_hi"] and d[f"{first}_se"] > 0
    # num_users=None reads the largest id; ids beyond the users with samples add nothing
    _same_dict(compute_bootstrap_ranking(u, y, _dev(s), ks, R, 2, None, True),
               compute_bootstrap_ranking(u, y, _dev(s), ks, R, 2, U + 500, True))


def test_the_order_of_the_samples_does_not_matter():
    """Any permutation when no two scores of a user tie; with ties, any permutation that keeps each user's samples in
    their order (a user's rank is defined by the dataset order of its tied samples)."""
    from deepfm_amd.training import compute_bootstrap_ranking
    rng = np.random.default_rng(41)
    U, R, ks = 400, 33, [1, 5]
    u, y, s = _population(rng, U, 30, "contiguous", ties=False)
    p = rng.permutation(u.size)
    _same_dict(compute_bootstrap_ranking(u, y, _dev(s), ks, R, 7, U, True),
               compute_bootstrap_ranking(u[p], y[p], _dev(s[p]), ks, R, 7, U, True))
    u, y, s = _population(rng, U, 30, "contiguous")
    shuffled = u[rng.permutation(u.size)]                                   # where each user's samples go ...
    p = np.empty(u.size, np.int64)
    p[np.argsort(shuffled, kind="stable")] = np.argsort(u, kind="stable")  # ... in the order they had
    assert np.array_equal(u[p], shuffled) and not np.array_equal(shuffled, u)
    _same_dict(compute_bootstrap_ranking(u, y, _dev(s), ks, R, 7, U, True),
               compute_bootstrap_ranking(u[p], y[p], _dev(s[p]), ks, R, 7, U, True))


def test_one_user_drops_the_replicates_that_weigh_it_zero():
    from deepfm_amd.training import compute_bootstrap_ranking
    R = 64
    u = np.zeros(6, np.int64)
    y = np.array([0, 1, 0, 0, 1, 0], np.float32)
    s = np.array([.9, .8, .7, .6, .5, .4], np.float32)
    d = compute_bootstrap_ranking(u, y, _dev(s), [1, 2], R, seed=1, group_auc=True)
    live = int((np.array([BR.weights(1, r, np.array([0]))[0] for r in range(R)]) > 0).sum())
    assert 0 < live < R
    for m in UR.names([1, 2], True):
        # every live replicate is the point value (NDCG: in fixed point)
        # (np.std of equal values: 0 up to the rounding of their mean)
        assert d[f"{m}_replicates"] == live and d[f"{m}_lo"] == d[f"{m}_hi"] and d[f"{m}_se"] <= 1e-15, m
        assert abs(d[f"{m}_lo"] - d[m]) <= (RESOLUTION if m.startswith("NDCG") else 0.0), m
    assert (d["HR@1"], d["HR@2"], d["uauc"]) == (0.0, 1.0, 0.5)


def test_compare_pairs_the_two_vectors_under_one_resampling():
    from deepfm_amd.training import compare_bootstrap_ranking, compute_bootstrap_ranking
    rng = np.random.default_rng(42)
    U, R, ks = 500, 48, [1, 5]
    u, y, sa = _population(rng, U, 30, "interleaved", ties=False)
    sb = (sa + 0.7 * (y - 0.5)).astype(np.float32)                          # b is the better scorer
    names = UR.names(ks, True)
    suffixes = ("a", "b", "delta", "delta_se", "delta_lo", "delta_hi", "b_better")
    same = compare_bootstrap_ranking(u, y, _dev(sa), _dev(sa), ks, R, 6, U, True)
    assert list(same) == [f"{m}_{k}" for m in names for k in suffixes]
    for m in names:
        assert same[f"{m}_a"] == same[f"{m}_b"]
        assert [same[f"{m}_delta{k}"] for k in ("", "_se", "_lo", "_hi")] == [0.0] * 4 and same[f"{m}_b_better"] == 0.0
    d = compare_bootstrap_ranking(u, y, _dev(sa), _dev(sb), ks, R, 6, U, True, level=0.9)
    a, b = compute_bootstrap_ranking(u, y, _dev(sa), ks, R, 6, U, True), compute_bootstrap_ranking(u, y, _dev(sb), ks, R,
                                                                                                   6, U, True)
    delta = UR.bootstrap_grouped(u, y, sb, ks, R, 6, U, True) - UR.bootstrap_grouped(u, y, sa, ks, R, 6, U, True)
    spread = UR.summary(delta, names, 0.9)
    for j, m in enumerate(names):
        assert (d[f"{m}_a"], d[f"{m}_b"], d[f"{m}_delta"]) == (a[m], b[m], b[m] - a[m])
        assert [d[f"{m}_delta_{k}"] for k in ("se", "lo", "hi")] == [spread[f"{m}_{k}"] for k in ("se", "lo", "hi")]
        assert d[f"{m}_b_better"] == np.mean(delta[:, j] > 0) and d[f"{m}_delta_lo"] > 0, m


def test_a_perfect_ranking_has_a_degenerate_interval():
    from deepfm_amd.training import compute_bootstrap_ranking
    rng = np.random.default_rng(43)
    u, y, _ = _population(rng, 200, 20, "interleaved")
    s = (y + 0.25 * rng.random(u.size)).astype(np.float32)                  # every positive in front of every negative
    d = compute_bootstrap_ranking(u, y, _dev(s), [1, 5], 40, seed=8, group_auc=True)
    for m in ("HR@1", "NDCG@1", "HR@5", "uauc", "gauc"):
        assert (d[m], d[f"{m}_lo"], d[f"{m}_hi"], d[f"{m}_se"]) == (1.0, 1.0, 1.0, 0.0), m


# ----------------------------------------------------------------------------- the predictors
def _check_predictor(pred, cols, uid, loader, ks):
    from deepfm_amd.training import compute_bootstrap_ranking
    R = 40
    duid = torch.from_numpy(uid).cuda()
    for how in ("evaluate", "evaluate_loader"):
        run = (lambda **kw: pred.evaluate(cols, **kw)) if how == "evaluate" else \
            (lambda **kw: pred.evaluate_loader(loader, **kw))
        for kw, cut, group_auc in ((dict(ranking_ks=ks, group_auc=True), ks, True), (dict(ranking_ks=ks), ks, False),
                                   (dict(group_auc=True), [], True)):
            today = run(bootstrap=R, bootstrap_by="user_id", bootstrap_seed=3, **kw)
            assert not any("@" in k and k.endswith("_se") for k in today) and "gauc_se" not in today, how
            m = run(bootstrap=R, bootstrap_by="user_id", bootstrap_seed=3, bootstrap_grouped=True, **kw)
            new = _spread_keys(UR.names(cut, group_auc))
            assert list(m) == list(today) + new and {k: m[k] for k in today} == today, how
            want = compute_bootstrap_ranking(duid, pred.last_labels, pred.last_scores, cut, R, 3, None, group_auc)
            _same_dict({k: m[k] for k in new}, {k: want[k] for k in new})
            assert all(m[k] == want[k] for k in want if k not in new), how
            ref = UR.bootstrap_grouped(uid, pred.last_labels.cpu().numpy(), pred.last_scores.cpu().numpy(), cut, R, 3,
                                       None, group_auc)
            _same_dict({k: m[k] for k in new}, UR.summary(ref, UR.names(cut, group_auc)))
    with pytest.raises(ValueError, match="bootstrap_grouped .* needs bootstrap "):
        pred.evaluate(cols, ranking_ks=ks, bootstrap_grouped=True)
    with pytest.raises(ValueError, match="needs bootstrap_by == user_field"):
        pred.evaluate_loader(loader, ranking_ks=ks, bootstrap=10, bootstrap_grouped=True)
    with pytest.raises(ValueError, match="needs ranking_ks or group_auc"):
        pred.evaluate(cols, bootstrap=10, bootstrap_by="user_id", bootstrap_grouped=True)


def test_mixed_predictor_adds_the_grouped_intervals():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import MixedSchemaPredictor
    from tests.helpers import random_fields_batch
    from tests.test_gpu_mixed_predict import _movielens_model
    fields, model = _movielens_model("deepfm", seed=5)
    U, C, B = 60, 50, 512
    n = U * C
    rng = np.random.default_rng(13)
    feats = random_fields_batch(fields, n, rng, zero_frac=0.05)
    feats["user_id"] = np.repeat(np.arange(1, U + 1, dtype=np.int64), C)
    labels = (rng.random(n) < 0.2).astype(np.float32)
    cols = PackedColumns(model.schema, feats, labels)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    _check_predictor(MixedSchemaPredictor(model, B), cols, feats["user_id"], loader, [1, 5, 10])


def test_uniform_predictor_adds_the_grouped_intervals():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FusedPredictor
    from tests.test_gpu_ranking import _user_model
    model = _user_model()
    users, cands, B = 90, 40, 512
    rng = np.random.default_rng(11)
    uid = np.repeat(np.arange(users, dtype=np.int64) * 7, cands)
    y = (rng.random(uid.size) < 0.25).astype(np.float32)
    feats = {"user_id": uid, "item_id": rng.integers(0, 5000, uid.size), "genre": rng.integers(0, 20, uid.size),
             "age": rng.random(uid.size).astype(np.float32)}
    cols = PackedColumns(model.schema, feats, y)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    _check_predictor(FusedPredictor(model, B), cols, uid, loader, [1, 5])


# ----------------------------------------------------------------------------- the Trainer
def test_trainer_reports_the_grouped_intervals_of_the_test_split_only(tmp_path):
    import deepfm_amd.training as T
    from tests.test_gpu_trainer import _trainer_config, _trainer_data, _trainer_model
    cfg = _trainer_config(tmp_path / "run", num_epochs=1)
    schema, (train, val, test) = _trainer_data(cfg)
    trainer = T.Trainer(_trainer_model(schema, cfg), schema, cfg, train, val, test, bootstrap=40, bootstrap_grouped=True)
    got = trainer.train()
    with open(tmp_path / "run" / "results.json") as f:
        res = json.load(f)
    new = _spread_keys(UR.names(cfg.training.ranking_ks, False))
    assert res["val_metrics"] == got and not set(new) & set(got)
    m = res["test_metrics"]
    assert set(new) <= set(m) and "auc_se" in m and "gauc_se" not in m
    for k in cfg.training.ranking_ks:
        assert m[f"HR@{k}_replicates"] == m[f"NDCG@{k}_replicates"] == 40
        assert 0 <= m[f"HR@{k}_lo"] <= m[f"HR@{k}"] <= m[f"HR@{k}_hi"] <= 1
    assert m["HR@10_se"] > 0
