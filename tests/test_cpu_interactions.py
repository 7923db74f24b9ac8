"""CPU: the numpy restatement of the interaction log (``tests/interactions_reference.py``) against what the reference's
own adapter methods gave (``tests/golden/interactions_reference.npz``, ``tools/make_interactions_golden.py``), the cutoff
arithmetic against numpy's percentile, the host-side refusals of ``deepfm_amd/data/interactions.py`` by message, and
the two host-side feature functions against the fixture bit for bit.  No GPU and no built library needed."""
import os

import numpy as np
import pytest
import torch

from deepfm_amd import _lib
from deepfm_amd.data import DeviceInteractionLog, SeenSets, count_feature_table, item_weights, popularity_weights
from deepfm_amd.data import interactions as I
from tests import interactions_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interactions_reference.npz")
RATIOS = [(0.1, 0.1), (0.15, 0.05), (0.2, 0.2), (0, 0.1)]


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_has_the_inputs_it_promises(G):
    """No user has two rows at one timestamp (the reference's answer is unique); users tie with each other, and every
    cutoff falls inside a run of equal timestamps."""
    u, ts = G["user_rows"], G["timestamps"]
    assert len(u) <= 400 and len(np.unique(np.stack([u, ts], 1), axis=0)) == len(u)
    assert len(np.unique(ts)) < len(ts) // 2
    s, n = np.sort(ts), len(ts)
    for k in range(4):
        v, t = float(G[f"temporal/{k}/val_ratio"]), float(G[f"temporal/{k}/test_ratio"])
        for q in (1 - v - t, 1 - t):
            lo = int(np.floor(q * (n - 1)))
            assert s[lo - 1] == s[lo] == s[lo + 1], (k, q)
    assert np.array_equal(G["labels"], (G["ratings"] >= G["label_threshold"]).astype(np.float32))
    sizes = np.bincount(u, minlength=int(G["n_users"]))
    assert {1, 2, 3} <= set(sizes.tolist())                       # below, at and above the leave-one-out thresholds


@pytest.mark.parametrize("k", range(4))
def test_restated_temporal_split_equals_the_reference(G, k):
    v, t = float(G[f"temporal/{k}/val_ratio"]), float(G[f"temporal/{k}/test_ratio"])
    assert (v, t) == tuple(map(float, RATIOS[k]))
    train, val, test, _ = R.temporal_split(G["user_rows"], G["timestamps"], G["labels"], v, t)
    # pandas' order inside a run of equal timestamps is unspecified: train as a set, the per-user parts exactly
    assert np.array_equal(np.sort(train), np.sort(G[f"temporal/{k}/train"]))
    assert np.array_equal(val, G[f"temporal/{k}/val"]) and np.array_equal(test, G[f"temporal/{k}/test"])
    assert np.array_equal(G["timestamps"][train], np.sort(G["timestamps"][train]))
    assert len(test) > 0 and (len(val) > 0) == (v > 0)


@pytest.mark.parametrize("m", [2, 3])
def test_restated_leave_one_out_split_equals_the_reference(G, m):
    parts = R.leave_one_out_split(G["user_rows"], G["timestamps"], m)
    for got, name in zip(parts, ("train", "val", "test")):
        assert np.array_equal(got, G[f"loo/{m}/{name}"]), name
    assert len(parts[1]) == len(parts[2]) == int((np.bincount(G["user_rows"]) >= m).sum())


def test_restated_seen_sets_and_counts_equal_the_reference(G):
    n_users, n_items = int(G["n_users"]), int(G["n_items"])
    assert np.array_equal(R.seen_pairs(G["user_rows"], G["item_rows"]), G["user_items"])
    seen = SeenSets.from_interactions(G["user_rows"], G["item_rows"], n_users, n_items)
    assert np.array_equal(R.pairs_of_bitmap(seen.bitmap, n_items), G["user_items"])
    assert len(G["user_items"]) < len(G["user_rows"])             # duplicated interactions are in the log
    for prefix in ("temporal/0", "loo/3"):
        train = G[f"{prefix}/train"]
        assert np.array_equal(R.entity_counts(G["user_rows"], n_users, G["labels"], train), G[f"{prefix}/user_counts"])
        assert np.array_equal(R.entity_counts(G["item_rows"], n_items, G["labels"], train), G[f"{prefix}/item_counts"])
        # _build_popularity_weights at alpha = 1 is max(count, 1) per item of the catalogue
        assert np.array_equal(np.maximum(G[f"{prefix}/item_counts"], 1).astype(np.float64),
                              G[f"{prefix}/pop_weights_alpha1"])


@pytest.mark.parametrize("prefix", ["temporal/0", "loo/3"])
def test_count_feature_table_and_popularity_weights_bit_for_bit(G, prefix):
    for by, rows in (("user", G["user_rows"]), ("item", G["item_rows"])):
        counts = G[f"{prefix}/{by}_counts"]
        want = G[f"{prefix}/{by}_rating_count"]
        assert (counts == 0).any() and want.dtype == np.float32
        for source in (counts, torch.from_numpy(counts)):
            table = count_feature_table(source)
            assert table.dtype == np.float32 and table.shape == counts.shape
            assert np.array_equal(table[rows].view(np.uint32), want.view(np.uint32)), by
        assert np.array_equal(R.count_feature_table(counts).view(np.uint32), count_feature_table(counts).view(np.uint32))
        on_cpu = count_feature_table(counts, device="cpu")
        assert isinstance(on_cpu, torch.Tensor) and np.array_equal(on_cpu.numpy(), count_feature_table(counts))
    item_counts = G[f"{prefix}/item_counts"]
    for alpha in (0.75, 1.0, 0.0):
        want = item_weights(item_counts, alpha)
        assert np.array_equal(popularity_weights(item_counts, alpha), want)
        assert np.array_equal(popularity_weights(torch.from_numpy(item_counts), alpha), want)
    # every count equal: max == min, all zeros
    assert np.array_equal(count_feature_table(np.array([3, 3, 0, 3])), np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="no entity has a count"):
        count_feature_table(np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="non-negative integers"):
        count_feature_table(np.array([1.0, 2.0]))


# ---------------------------------------------------------------------------------------------------- the cutoffs
def test_cutoff_arithmetic_equals_numpy_percentile():
    """n = 1..300 x four ratio pairs x both cutoffs, on columns with ties and with wide gaps: the float64 value from
    two order statistics is bitwise numpy's (and so pandas')."""
    rng = np.random.default_rng(7)
    cases = 0
    for n in range(1, 301):
        columns = (np.sort(rng.integers(0, 50, n)), np.sort(rng.integers(-2**52, 2**52, n)),
                   np.sort(874724710 + rng.integers(0, 10**7, n)))
        for v, t in RATIOS:
            for q in (1 - v - t, 1 - t):
                lo, hi, g = I.quantile_position(q, n)
                assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= g < 1.0 or lo == hi == n - 1
                for col in columns:
                    col = col.astype(np.int64)
                    want = np.percentile(col, q * 100.0, method="linear")
                    got = I.quantile_cutoff(col[lo], col[hi], g)
                    assert got == want and R.quantile(col, q) == want, (n, v, t, q)
                    cases += 1
    assert cases == 300 * 4 * 2 * 3


# ---------------------------------------------------------------------------------------------------- refusals
def _columns(n=5):
    return (np.arange(n, dtype=np.int64) % 3, np.arange(n, dtype=np.int64) % 4, np.arange(n, dtype=np.int64) + 10,
            np.ones(n, np.float32))


def test_host_refusals_by_message():
    """Each is raised before anything touches a device (there is none here for most runs of this test)."""
    u, i, ts, lab = _columns()
    with pytest.raises(ValueError, match="differ in length"):
        DeviceInteractionLog(u, i[:4], ts, lab, 3, 4)
    with pytest.raises(ValueError, match="differ in length"):
        DeviceInteractionLog(u, i, ts, lab[:1], 3, 4)
    huge = np.broadcast_to(np.zeros(1, np.int64), (2**31,))                     # a header, not 16 GiB
    with pytest.raises(ValueError, match="fewer than 2\\^31"):
        DeviceInteractionLog(huge, huge, huge, np.broadcast_to(np.zeros(1, np.float32), (2**31,)), 3, 4)
    for bad in (2**53, -2**53):
        t2 = ts.copy(); t2[3] = bad
        with pytest.raises(ValueError, match=r"timestamps\[3\] = -?\d+: \|timestamp\| must be below 2\^53"):
            DeviceInteractionLog(u, i, t2, lab, 3, 4)
        with pytest.raises(ValueError, match=r"timestamps\[3\]"):
            DeviceInteractionLog(u, i, torch.from_numpy(t2), lab, 3, 4)
    # the seen-set size rule, in SeenSets.from_interactions' own words
    for n_users, n_items in ((1 << 20, 1 << 16), (0, 4), (3, 0)):
        with pytest.raises(ValueError) as host:
            SeenSets.from_interactions(u, i, n_users, n_items)
        with pytest.raises(ValueError) as dev:
            DeviceInteractionLog(u, i, ts, lab, n_users, n_items)
        assert str(dev.value) == str(host.value)
    assert "needs another structure" in str(dev.value) or "must be positive" in str(dev.value)
    with pytest.raises(TypeError, match="user_rows: expected torch.int64"):
        DeviceInteractionLog(u.astype(np.int32), i, ts, lab, 3, 4)
    with pytest.raises(TypeError, match="labels: expected torch.float32"):
        DeviceInteractionLog(u, i, ts, lab.astype(np.float64), 3, 4)
    with pytest.raises(ValueError, match="one axis"):
        DeviceInteractionLog(u.reshape(1, -1), i, ts, lab, 3, 4)
    with pytest.raises(TypeError, match="numpy array"):
        DeviceInteractionLog(u.tolist(), i, ts, lab, 3, 4)


@pytest.mark.parametrize("ratios", [(-0.1, 0.1), (0.1, -0.1), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.6, 0.7),
                                    (float("nan"), 0.1), ("0.1", 0.1)])
def test_ratios_outside_the_simplex_are_refused(ratios):
    with pytest.raises(ValueError, match="both must lie in \\[0, 1\\) and their sum below 1"):
        I._check_ratios(*ratios)
    # the method refuses before it sorts: a log object without any device state is enough to see that
    log = DeviceInteractionLog.__new__(DeviceInteractionLog)
    with pytest.raises(ValueError, match="both must lie"):
        log.temporal_split(*ratios)


def test_min_interactions_below_two_is_refused():
    log = DeviceInteractionLog.__new__(DeviceInteractionLog)
    for bad in (1, 0, -3, 2.5):
        with pytest.raises(ValueError, match="at least 2"):
            log.leave_one_out_split(bad)
    for ok in RATIOS:
        I._check_ratios(*ok)


def test_quantile_position_refuses_nonsense():
    with pytest.raises(ValueError, match="empty column"):
        I.quantile_position(0.5, 0)
    with pytest.raises(ValueError, match="outside \\[0, 1\\]"):
        I.quantile_position(1.5, 10)
    assert I.quantile_position(1.0, 7) == (6, 6, 0.0) and I.quantile_position(0.3, 1) == (0, 0, 0.0)


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_new_signatures_are_present_and_the_abi_version_is_the_bindings():
    for name in ("dfm_seen_sets_build", "dfm_entity_counts", "dfm_temporal_split_mark", "dfm_loo_split_mark"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "deepfm_hip.h")).read()
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        if name.startswith(("dfm_seen_sets", "dfm_entity_counts", "dfm_temporal_split", "dfm_loo_split")):
            decl = header[header.index(f"int {name}("):]
            decl = decl[:decl.index(");")]
            assert decl.count(",") + 1 == len(argtypes), name
    assert _lib.load().dfm_abi_version() == _lib.ABI_VERSION
    assert f"#define DFM_ABI_VERSION {_lib.ABI_VERSION} " in header
    assert f"#define DFM_COUNTS_LDS_ENTITIES {_lib.COUNTS_LDS_ENTITIES}\n" in header
