"""GPU: the grouped AUC (csrc/grouped_auc.hip) against the numpy restatement (tests/grouped_auc_reference.py), bit for
bit: per-group ``auc_g``, ``gauc``, ``uauc`` and the counts; against sklearn per group within 1e-12; independence of
the sample order; through the predictors' ``evaluate`` / ``evaluate_loader`` and the Trainer."""
import json

import numpy as np
import pytest
import torch

from tests import grouped_auc_reference as GR

pytestmark = pytest.mark.gpu


def _device(group_ids, labels, scores, num_groups=None):
    from deepfm_amd.training import grouped_auc_device
    out, per_group = grouped_auc_device(group_ids, labels, scores, num_groups, per_group=True)
    return out, per_group


def _check(group_ids, labels, scores, num_groups=None, what=""):
    """The device values of one input against the restatement, bit for bit; returns (out, per_group, restatement)."""
    from deepfm_amd.training import compute_gauc
    out, per_group = _device(group_ids, labels, scores, num_groups)
    want = GR.grouped_auc(group_ids, labels, scores, num_groups)
    got = out.cpu().numpy()
    pg = per_group.cpu().numpy()
    print(f"{what}: groups {got[0]:.0f} gauc {got[1]!r} / {want['gauc']!r} uauc {got[2]!r} / {want['uauc']!r}")
    assert pg.shape == want["per_group"].shape
    both_nan = np.isnan(pg) & np.isnan(want["per_group"])
    assert np.all((pg == want["per_group"]) | both_nan), what           # == on the doubles
    assert got[0] == want["groups"] and got[3] == want["samples"], what
    assert got[4:].tolist() == [want["bad_id"], want["nan"], want["bad_label"]], what
    if want["groups"]:
        assert got[1] == want["gauc"] and got[2] == want["uauc"], what
    else:
        assert np.isnan(got[1]) and np.isnan(got[2]), what
    if not (want["bad_id"] or want["nan"] or want["bad_label"]):
        d = compute_gauc(group_ids, labels, scores, num_groups)
        assert d == ({"gauc": want["gauc"], "uauc": want["uauc"]} if want["groups"] else {}), what
        assert all(type(v) is float for v in d.values())
    return out, per_group, want


def _check_sklearn(group_ids, labels, scores, per_group, out=None):
    from sklearn.metrics import roc_auc_score
    g, y, s = (np.asarray(x) for x in (group_ids, labels, scores))
    pg = per_group.cpu().numpy()
    aucs, weights = [], []
    for gid in np.unique(g):
        m = g == gid
        if 0 < y[m].sum() < m.sum():
            want = roc_auc_score(y[m], s[m])
            assert abs(pg[gid] - want) <= 1e-12, gid
            aucs.append(want)
            weights.append(int(m.sum()))
    if out is None:
        return
    got = out.cpu().numpy()
    assert got[0] == len(aucs)
    assert abs(got[1] - np.average(aucs, weights=weights)) <= 1e-12 and abs(got[2] - np.mean(aucs)) <= 1e-12


def _split(rng, lengths, levels=None, pos_rate=0.3):
    g = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    s = rng.standard_normal(g.size).astype(np.float32)
    if levels:
        s = (np.floor(rng.random(g.size) * levels) / levels).astype(np.float32)
    y = (rng.random(g.size) < pos_rate).astype(np.float32)
    return g, y, s


def _stride_permutation(n, stride):
    p = (np.arange(n, dtype=np.int64) * stride) % n
    assert np.unique(p).size == n
    return p


def test_one_sample():
    from deepfm_amd.training import compute_gauc
    for y in (0.0, 1.0):
        out, pg, want = _check(np.array([0]), np.array([y], np.float32), np.array([0.3], np.float32), what=f"n=1 y={y}")
        assert want["groups"] == 0 and np.isnan(pg.cpu().numpy()).all()
    assert compute_gauc(np.array([0]), np.array([1.0], np.float32), np.array([0.3], np.float32)) == {}


def test_one_group_of_one_class_gives_no_keys():
    from deepfm_amd.training import compute_gauc
    rng = np.random.default_rng(0)
    s = rng.random(300).astype(np.float32)
    g = np.zeros(300, np.int64)
    for y in (np.zeros(300, np.float32), np.ones(300, np.float32)):
        _check(g, y, s, what="one class")
        assert compute_gauc(torch.from_numpy(g).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()) == {}


def test_two_groups_of_which_one_qualifies():
    g = np.array([0, 0, 0, 1, 1, 1, 1])
    y = np.array([1, 1, 1, 0, 1, 0, 1], np.float32)
    s = np.array([.5, .1, .2, .4, .4, .1, .9], np.float32)
    out, pg, want = _check(g, y, s, what="two groups")
    assert want["groups"] == 1 and want["samples"] == 4
    pg = pg.cpu().numpy()
    assert np.isnan(pg[0]) and pg[1] == 7 / 8              # pairs: .4>.1, .4==.4, .9>.4, .9>.1 -> (2*3 + 1) / 8
    assert out.cpu().tolist()[1:3] == [7 / 8, 7 / 8]


# group sizes at the wave (64) and workgroup (256) edges and one group across several workgroups
_EDGES = [1, 2, 63, 64, 65, 255, 256, 257, 1025]


@pytest.mark.parametrize("levels", [None, 4], ids=["distinct", "four_values"])
def test_wave_and_workgroup_edges_contiguous_and_interleaved(levels):
    rng = np.random.default_rng(3)
    g, y, s = _split(rng, _EDGES, levels=levels, pos_rate=0.4)
    y[0] = 1.0                                             # the group of one sample: never qualifies
    y[1:3] = [0.0, 1.0]                                    # the group of two: one pair
    out, pg, want = _check(g, y, s, what=f"edges contiguous levels={levels}")
    assert want["groups"] == len(_EDGES) - 1
    _check_sklearn(g, y, s, pg, out)
    p = _stride_permutation(g.size, 997)
    assert np.any(np.diff(g[p]) < 0)
    out2, pg2, _ = _check(g[p], y[p], s[p], what="edges interleaved")
    assert torch.equal(out, out2) and torch.equal(pg.nan_to_num(nan=-1.0), pg2.nan_to_num(nan=-1.0))


def test_all_scores_equal_gives_exactly_one_half():
    rng = np.random.default_rng(4)
    g, y, _ = _split(rng, [5, 64, 300, 1, 77], pos_rate=0.5)
    s = np.full(g.size, 0.25, np.float32)
    out, pg, want = _check(g, y, s, what="all equal")
    pg = pg.cpu().numpy()
    keep = ~np.isnan(pg)
    assert keep.sum() == want["groups"] >= 3 and np.all(pg[keep] == 0.5)
    assert out.cpu().tolist()[1:3] == [0.5, 0.5]


def test_signed_zero_infinite_and_denormal_scores():
    # group 0: -0.0 against +0.0 is a tie; group 1: +-inf; group 2: denormals order by value, apart from zero
    tiny = np.float32(1e-45)
    g = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2])
    y = np.array([1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1], np.float32)
    s = np.array([-0.0, 0.0, -0.0, 0.0, np.inf, np.inf, -np.inf, -np.inf, 3e38,
                  tiny, 0.0, -tiny, -0.0, 2 * tiny, 2 * tiny], np.float32)
    assert s[9] > 0 and s[11] < 0
    out, pg, want = _check(g, y, s, what="special values")
    pg = pg.cpu().numpy()
    assert pg[0] == 0.5
    assert pg[1] == (2 * 2 + 1 + 0 + 1) / 12               # +inf: beats two, ties one; -inf: ties one
    assert pg[2] == (2 * 2 + 0 + 2 * 2 + 1) / 18           # tiny > both zeros; -tiny < all; 2 tiny: > zeros, ties one
    m = g != 1                                             # sklearn refuses infinite scores
    _check_sklearn(g[m], y[m], s[m], torch.from_numpy(pg))


def test_sparse_ids_far_below_num_groups():
    rng = np.random.default_rng(5)
    num_groups = 1_000_003                                 # several rounds of the leaves of 1024 workgroups
    ids = np.sort(rng.choice(num_groups - 1, 400, replace=False))
    ids[-1] = num_groups - 1
    g, y, s = _split(rng, [37] * 400, levels=16)
    g = ids[g]
    p = rng.permutation(g.size)
    g, y, s = g[p], y[p], s[p]
    out, pg, want = _check(g, y, s, num_groups, what="sparse ids")
    assert want["groups"] >= 390 and not np.isnan(want["per_group"][num_groups - 1])
    assert int((~torch.isnan(pg)).sum()) == want["groups"]
    # absent groups add zeros to the fixed tree: the values do not depend on num_groups
    out_d, _, _ = _check(g, y, s, None, what="sparse ids, default num_groups")
    out_w, pg_w, _ = _check(g, y, s, 2_000_000, what="sparse ids, a wider num_groups")
    assert torch.equal(out_d, out) and torch.equal(out_w, out) and bool(torch.isnan(pg_w[num_groups:]).all())


def test_one_group_holds_the_whole_input():
    rng = np.random.default_rng(6)
    n = 50_000
    g = np.zeros(n, np.int64)
    y = (np.arange(n) % 2).astype(np.float32)
    rng.shuffle(y)
    s = (rng.standard_normal(n) + 0.3 * y).astype(np.float32)
    s[::50] = np.float32(0.125)                            # a run of ties as well
    out, pg, want = _check(g, y, s, what="one group, n = 50000")
    assert want["groups"] == 1 and 0.5 < want["gauc"] < 0.7 and want["gauc"] == want["uauc"] == want["per_group"][0]
    from sklearn.metrics import roc_auc_score
    assert abs(float(pg[0]) - roc_auc_score(y, s)) <= 1e-12


def test_the_protocols_shape_and_order_independence():
    """943 groups of 1 positive + 999 negatives; two runs and a shuffled copy give the same bits."""
    rng = np.random.default_rng(7)
    U, C = 943, 1000
    g = np.repeat(np.arange(U, dtype=np.int64), C)
    y = np.zeros(U * C, np.float32)
    y[np.arange(U) * C + rng.integers(0, C, U)] = 1.0
    s = (np.floor(rng.random(U * C) * 4096) / 4096).astype(np.float32)      # some ties with the positive
    out, pg, want = _check(g, y, s, what="943 x 1000")
    assert want["groups"] == U and want["samples"] == U * C
    d = [torch.from_numpy(x).cuda() for x in (g, y, s)]
    again, pg_again = _device(*d)
    assert torch.equal(out, again) and torch.equal(pg, pg_again)
    p = torch.from_numpy(rng.permutation(U * C)).cuda()
    shuffled, pg_shuffled = _device(d[0][p], d[1][p], d[2][p])
    assert torch.equal(out, shuffled) and torch.equal(pg, pg_shuffled)
    # every group has one positive: auc_g = 1 - rank / 999 with half ranks for ties
    k = GR.ord_bits(s).astype(np.int64).reshape(U, C)
    yp = y.reshape(U, C) == 1
    sp = k[yp][:, None]
    expect = (2 * ((k < sp) & ~yp).sum(1) + ((k == sp) & ~yp).sum(1)) / (2.0 * 999)
    assert np.array_equal(pg.cpu().numpy(), expect)


@pytest.mark.parametrize("bad", ["id_high", "id_negative", "nan", "label_half"])
def test_invalid_samples_raise_with_their_count(bad):
    from deepfm_amd.training import compute_gauc
    rng = np.random.default_rng(8)
    g, y, s = _split(rng, [20] * 100)
    if bad == "id_high":
        g[[5, 700, 1999]] = 100
        msg = r"^3 group ids outside \[0, num_groups\)$"
    elif bad == "id_negative":
        g[[17, 18]] = -4
        msg = r"^2 group ids outside \[0, num_groups\)$"
    elif bad == "nan":
        s[[1, 2, 3, 1500]] = np.nan
        msg = r"^Input contains NaN\.$"
    else:
        y[77] = 0.5
        msg = r"^1 labels other than 0 and 1$"
    with pytest.raises(ValueError, match=msg):
        compute_gauc(g, y, s, num_groups=100)
    _check(g, y, s, 100, what=f"{bad}: counted, not used")


def test_invalid_samples_leave_the_other_groups_alone_direct_abi():
    """prepare -> sort -> finish through the C ABI: with invalid samples mixed in, every value equals the clean
    input's, and the three counts are theirs."""
    from deepfm_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(9)
    G = 300
    g, y, s = _split(rng, [33] * G, levels=8)
    extra = 500
    xg = rng.integers(0, G, extra)
    xy = (rng.random(extra) < 0.5).astype(np.float32)
    xs = rng.standard_normal(extra).astype(np.float32)
    xg[:200] = np.where(rng.random(200) < 0.5, G + rng.integers(0, 10**12, 200), -1 - rng.integers(0, 10**12, 200))
    xs[200:350] = np.nan
    xy[350:] = rng.choice(np.array([0.5, -1.0, 2.0, np.nan, 1.0000001], np.float32), 150)
    p = rng.permutation(g.size + extra)

    def run(gi, yi, si):
        n = gi.size
        d_g, d_y, d_s = torch.from_numpy(gi).cuda(), torch.from_numpy(yi).cuda(), torch.from_numpy(si).cuda()
        keys = torch.empty(n, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.dfm_grouped_auc_workspace_bytes(n, G), dtype=torch.uint8, device="cuda")
        st = _lib.stream_handle()
        _lib.check(lib.dfm_grouped_auc_prepare(d_g.data_ptr(), d_y.data_ptr(), d_s.data_ptr(), n, G, keys.data_ptr(),
                                               ws.data_ptr(), st))
        ordered = torch.sort(keys).values
        out = torch.full((7,), -1.0, dtype=torch.float64, device="cuda")
        pg = torch.full((G,), -1.0, dtype=torch.float64, device="cuda")
        _lib.check(lib.dfm_grouped_auc_finish(ordered.data_ptr(), n, G, ws.data_ptr(), pg.data_ptr(), out.data_ptr(), st))
        none = torch.full((7,), -1.0, dtype=torch.float64, device="cuda")     # without the per-group output
        _lib.check(lib.dfm_grouped_auc_finish(ordered.data_ptr(), n, G, ws.data_ptr(), None, none.data_ptr(), st))
        assert torch.equal(out, none)
        return out.cpu(), pg.cpu(), keys.cpu()

    clean_out, clean_pg, _ = run(g, y, s)
    out, pg, keys = run(np.concatenate([g, xg])[p], np.concatenate([y, xy])[p], np.concatenate([s, xs])[p])
    assert clean_out[4:].tolist() == [0.0, 0.0, 0.0] and out[4:].tolist() == [200.0, 150.0, 150.0]
    assert torch.equal(out[:4], clean_out[:4])
    assert torch.equal(pg.nan_to_num(nan=-2.0), clean_pg.nan_to_num(nan=-2.0))
    assert int((keys == torch.iinfo(torch.int64).max).sum()) == extra
    want = GR.grouped_auc(g, y, s, G)
    assert out[1] == want["gauc"] and out[2] == want["uauc"] and out[0] == want["groups"]


# ----------------------------------------------------------------------------- the predictors
def _check_predictor(pred, cols, uid, loader, ks, dense_field):
    from deepfm_amd.training import compute_gauc
    plain = pred.evaluate(cols, ranking_ks=ks)
    assert "gauc" not in plain and "uauc" not in plain
    assert list(pred.evaluate(cols)) == ["auc", "logloss"]
    for how in ("evaluate", "evaluate_loader"):
        if how == "evaluate":
            m = pred.evaluate(cols, ranking_ks=ks, group_auc=True)
        else:
            plain = pred.evaluate_loader(loader, ranking_ks=ks)
            m = pred.evaluate_loader(loader, ranking_ks=ks, group_auc=True)
        assert list(m) == list(plain) + ["gauc", "uauc"], how
        assert {k: m[k] for k in plain} == plain, how
        want = compute_gauc(torch.from_numpy(uid).cuda(), pred.last_labels, pred.last_scores)
        assert {"gauc": m["gauc"], "uauc": m["uauc"]} == want, how
        ref = GR.grouped_auc(uid, pred.last_labels.cpu().numpy(), pred.last_scores.cpu().numpy())
        assert m["gauc"] == ref["gauc"] and m["uauc"] == ref["uauc"], how
        assert 0.0 < m["gauc"] < 1.0
    only = pred.evaluate(cols, group_auc=True)                                # without the ranking metrics
    assert list(only) == ["auc", "logloss", "gauc", "uauc"] and only["gauc"] == m["gauc"]
    # no SPARSE field of that name (none at all, or a DENSE one): no key is added
    assert pred.model.schema.fields[dense_field].feature_type.name == "DENSE"
    assert list(pred.evaluate(cols, group_auc=True, user_field="visitor")) == ["auc", "logloss"]
    assert list(pred.evaluate_loader(loader, ranking_ks=ks, group_auc=True, user_field=dense_field)) == ["auc", "logloss"]


def test_mixed_predictor_adds_gauc_and_uauc():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import MixedSchemaPredictor
    from tests.helpers import random_fields_batch
    from tests.test_gpu_mixed_predict import _movielens_model
    fields, model = _movielens_model("deepfm", seed=5)
    U, C, B = 60, 50, 512
    n = U * C
    assert n % B
    rng = np.random.default_rng(13)
    feats = random_fields_batch(fields, n, rng, zero_frac=0.05)
    feats["user_id"] = np.repeat(np.arange(1, U + 1, dtype=np.int64), C)
    labels = (rng.random(n) < 0.2).astype(np.float32)
    labels[:C] = 0.0                                                          # a user of one class
    cols = PackedColumns(model.schema, feats, labels)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    _check_predictor(MixedSchemaPredictor(model, B), cols, feats["user_id"], loader, [1, 5, 10], "dow_sin")


def test_uniform_predictor_adds_gauc_and_uauc():
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
    _check_predictor(FusedPredictor(model, B), cols, uid, loader, [1, 5], "age")


# ----------------------------------------------------------------------------- the Trainer
@pytest.mark.parametrize("metric", ["gauc", "auc"])
def test_trainer_watches_the_configured_metric(tmp_path, metric):
    import deepfm_amd.training as T
    from deepfm_amd.utils.io import load_checkpoint
    from tests.test_gpu_trainer import _trainer_config, _trainer_data, _trainer_model
    cfg = _trainer_config(tmp_path / "run", metric=metric, num_epochs=2)
    schema, (train, val, test) = _trainer_data(cfg)
    trainer = T.Trainer(_trainer_model(schema, cfg), schema, cfg, train, val, test)
    seen = []
    inner = trainer.evaluate
    trainer.evaluate = lambda ds, split="eval": seen.append(inner(ds, split)) or seen[-1]
    got = trainer.train()
    ck = load_checkpoint(tmp_path / "run" / "best_model.pt")
    with open(tmp_path / "run" / "results.json") as f:
        res = json.load(f)
    assert len(seen) == 3 and got in seen[:2] and res["val_metrics"] == got and res["test_metrics"] == seen[2]
    if metric == "gauc":
        assert all({"auc", "logloss", "HR@1", "gauc", "uauc"} <= set(m) for m in seen)
        assert ck["best_metric"] == got["gauc"] == max(m["gauc"] for m in seen[:2])
        # the validation split is 40 users x (1 + 20): every user qualifies, so uauc == gauc up to the sums' rounding
        assert abs(got["gauc"] - got["uauc"]) <= 1e-12 and 0.0 < got["gauc"] <= 1.0
    else:
        assert all("gauc" not in m and "uauc" not in m for m in seen)
        assert ck["best_metric"] == got["auc"]
        assert "gauc" not in json.dumps(res["val_metrics"]) + json.dumps(res["test_metrics"])
