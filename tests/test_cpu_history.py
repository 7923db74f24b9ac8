"""CPU: the user histories of ``deepfm_amd/data/interactions.py`` (DESIGN.md §7b "User histories on the device").  The
two numpy restatements of ``tests/history_reference.py`` against each other and against the no-leak properties the
definition promises, every host-side refusal by message, ``history_field``, the two new C entry points' declarations
and argument checks, and the training limit the record backward's LDS cap puts on a history's length.  No GPU needed:
every refusal here is raised before any device work."""
import itertools
import os

import numpy as np
import pytest
import torch

from deepfm_amd import _lib
from deepfm_amd.data import DeviceHistoryIndex, DeviceInteractionLog, UserHistory, history_field
from deepfm_amd.data import interactions as I
from deepfm_amd.data.schema import FeatureType
from tests import history_reference as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_log(rng, n, n_users, n_items, ts_range=20):
    """Ties everywhere: ``ts_range`` timestamps for ``n`` rows."""
    return (rng.integers(0, n_users, n).astype(np.int64), rng.integers(0, n_items, n).astype(np.int64),
            rng.integers(-3, ts_range - 3, n).astype(np.int64), (rng.random(n) < 0.6).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("seed, n, n_users", [(0, 400, 7), (1, 150, 1), (2, 333, 40), (3, 1, 2)])
def test_the_two_restatements_agree(seed, n, n_users):
    rng = np.random.default_rng(seed)
    n_items = 30
    user, item, ts, labels = random_log(rng, n, n_users, n_items)
    half = rng.permutation(n)[:n // 2]
    ids = rng.integers(1, 1000, n_items).astype(np.int64)
    ids[[3, 11]] = 0
    options = itertools.product(H.TIES, (True, False), (None, np.concatenate([half, half[:5]])), (None, ids))
    for k, (ties, positives_only, source, item_ids) in enumerate(options):
        L = (1, 3, 50)[k % 3]
        queries = rng.integers(0, n_users if ties == "latest" else n, 25)
        kw = dict(ties=ties, source=source, positives_only=positives_only, item_ids=item_ids)
        got = H.histories(user, item, ts, labels, queries, L, **kw)
        want = H.histories_brute_force(user, item, ts, labels, queries, L, **kw)
        for g, w, name in zip(got, want, ("bag", "count", "gap")):
            assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (name, ties, positives_only, L)


@pytest.mark.parametrize("ties", ["position", "exclude"])
@pytest.mark.parametrize("positives_only", [True, False])
@pytest.mark.parametrize("with_source", [False, True])
def test_no_row_sees_itself_or_the_future(ties, positives_only, with_source):
    """Every row is its own item here, so a bag entry names the event it came from."""
    rng = np.random.default_rng(11)
    n, n_users, L = 400, 9, 6
    user, _, ts, labels = random_log(rng, n, n_users, n)
    item = np.arange(n, dtype=np.int64)
    source = rng.permutation(n)[:n // 2] if with_source else None
    queries = np.arange(n)
    bag, count, gap = H.histories(user, item, ts, labels, queries, L, ties=ties, source=source,
                                  positives_only=positives_only)
    filled = (bag != 0).sum(axis=1)
    assert np.array_equal(filled, np.minimum(L, count))           # min(L, count) ids ...
    assert all((bag[q, :filled[q]] != 0).all() for q in queries)  # ... and they lead
    assert np.array_equal(gap == -1, count == 0)
    assert (gap[count > 0] >= (0 if ties == "position" else 1)).all()
    assert (count > L).any() and (count == 0).any() and (count[labels == 0] > 0).any()
    for q in queries:
        events = bag[q, :filled[q]] - 1
        assert (user[events] == user[q]).all()
        if positives_only:
            assert (labels[events] == 1).all()
        if source is not None:
            assert np.isin(events, source).all()
        keys = [(int(ts[e]), int(e)) for e in events]
        assert keys == sorted(keys, reverse=True) and len(set(keys)) == len(keys)
        if ties == "position":
            assert all(k < (int(ts[q]), int(q)) for k in keys)
        else:
            assert all(k[0] < int(ts[q]) for k in keys)
        if len(keys):
            assert gap[q] == ts[q] - keys[0][0]


# ---------------------------------------------------------------------------------------------------- refusals
def _bare_log(n=6, n_users=3, n_items=4):
    """A log without any device state: enough to see that a refusal comes before the device is touched."""
    log = DeviceInteractionLog.__new__(DeviceInteractionLog)
    log.n, log.n_users, log.n_items, log.device = n, n_users, n_items, torch.device("cuda")
    return log


def _bare_index(n=6, n_users=3, n_items=4):
    ix = DeviceHistoryIndex.__new__(DeviceHistoryIndex)
    ix.n, ix.n_users, ix.n_items, ix.device = n, n_users, n_items, torch.device("cuda")
    return ix


def test_history_index_refusals_by_message():
    log = _bare_log()
    with pytest.raises(TypeError, match="source: expected torch.int64"):
        log.history_index(source=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="source: expected one axis"):
        log.history_index(source=torch.zeros(3, 1, dtype=torch.int64))
    with pytest.raises(TypeError, match="source: expected a torch tensor"):
        log.history_index(source=np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="source is on cpu, the log on cuda"):
        log.history_index(source=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError, match="item_ids: expected torch.int64"):
        log.history_index(item_ids=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match=r"item_ids: expected one id per item row, shape \(4,\)"):
        log.history_index(item_ids=np.zeros(5, np.int64))
    with pytest.raises(ValueError, match="item_ids: expected one axis"):
        log.history_index(item_ids=torch.zeros(4, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="item_ids: an id is negative"):
        log.history_index(item_ids=np.array([1, 2, -1, 0], np.int64))


@pytest.mark.parametrize("call", ["lookup", "latest"])
def test_lookup_and_latest_refusals_by_message(call):
    ix = _bare_index()
    what = "rows" if call == "lookup" else "user_rows"
    f = getattr(ix, call)
    good = torch.zeros(3, dtype=torch.int64)
    for bad in (0, -1, 4097, 2.0, True, None):
        with pytest.raises(ValueError, match=r"outside \[1, 4096\]"):
            f(good, bad)
    with pytest.raises(TypeError, match=f"{what}: expected torch.int64"):
        f(good.to(torch.int32), 5)
    with pytest.raises(ValueError, match=f"{what}: expected one axis"):
        f(good.reshape(3, 1), 5)
    with pytest.raises(TypeError, match=f"{what}: expected a torch tensor"):
        f(np.zeros(3, np.int64), 5)
    with pytest.raises(ValueError, match=f"{what} is on cpu, the log on cuda"):
        f(good, 5)
    # 4 GiB of bags is taken, one id more is not: the size is refused from the header of a tensor that holds one word
    m = I.HISTORY_MAX_BYTES // (8 * 4096)
    with pytest.raises(ValueError, match=f"more than {I.HISTORY_MAX_BYTES}: look the parts of {what} up separately"):
        f(torch.zeros(1, dtype=torch.int64).expand(m + 1), 4096)
    with pytest.raises(ValueError, match="is on cpu"):              # the next check: the size passed
        f(torch.zeros(1, dtype=torch.int64).expand(m), 4096)
    with pytest.raises(ValueError, match="fewer than 2\\^31"):
        f(torch.zeros(1, dtype=torch.int64).expand(2**31), 1)
    if call == "lookup":
        for ties in ("first", "", None, "latest"):
            with pytest.raises(ValueError, match="expected one of \\('position', 'exclude'\\)"):
                ix.lookup(good, 5, ties=ties)
    assert I.HISTORY_MAX_BYTES == 1 << 32 and I.HISTORY_TIES == ("position", "exclude")
    assert {f.name for f in UserHistory.__dataclass_fields__.values()} == {"bag", "count", "gap"}


def test_history_field_is_a_sequence_field_and_refuses_max_and_the_item_group():
    from deepfm_amd.data.device_epoch import Role, default_roles
    from deepfm_amd.data.schema import DatasetSchema
    spec = history_field("hist", 20, 1682, 16)
    assert (spec.name, spec.feature_type, spec.vocabulary_size, spec.embedding_dim, spec.group, spec.max_length,
            spec.combiner) == ("hist", FeatureType.SEQUENCE, 1683, 16, "user", 20, "mean")
    assert history_field("h", 1, 1, 8, combiner="sum", group="context").combiner == "sum"
    assert default_roles(DatasetSchema(fields={"hist": spec}))["hist"] is Role.COPY
    with pytest.raises(ValueError, match="field 'hist' pools with max: the embedding backward's arg-max recompute is "
                                         "not built"):
        history_field("hist", 20, 1682, 16, combiner="max")
    with pytest.raises(ValueError, match="group 'item' gives it the ITEM role"):
        history_field("hist", 20, 1682, 16, group="item")
    with pytest.raises(ValueError, match="expected 'mean' or 'sum'"):
        history_field("hist", 20, 1682, 16, combiner="median")
    for bad in (0, 4097):
        with pytest.raises(ValueError, match=r"outside \[1, 4096\]"):
            history_field("hist", bad, 1682, 16)
    with pytest.raises(ValueError, match="n_items = 0"):
        history_field("hist", 20, 0, 16)


# ---------------------------------------------------------------------------------------------------- the C ABI
NAMES = ("dfm_history_index_build", "dfm_history_gather")


def test_the_new_entry_points_are_declared_and_bound_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "deepfm_hip.h")).read()
    kinds = {"int64_t": _lib._L, "int": _lib._I, "dfm_stream_t": _lib._P}
    for name in NAMES:
        assert name in _lib.SIGNATURES
        restype, argtypes = _lib.SIGNATURES[name]
        decl = header[header.index(f"int {name}(") + len(f"int {name}("):]
        params = [p.strip() for p in decl[:decl.index(");")].split(",")]
        want = [_lib._P if "*" in p else kinds[p.rsplit(" ", 1)[0]] for p in params]
        assert restype is _lib._I and argtypes == want, name
        assert params[-1] == "dfm_stream_t stream"
    assert _lib.load().dfm_abi_version() == _lib.ABI_VERSION == 11
    assert "#define DFM_ABI_VERSION 11 " in header
    assert f"#define DFM_HISTORY_MAX_LENGTH {_lib.HISTORY_MAX_LENGTH} " in header
    assert "enum dfm_history_mode { DFM_HISTORY_POSITION = 0, DFM_HISTORY_EXCLUDE = 1, DFM_HISTORY_LATEST = 2 }" in header
    assert (_lib.HISTORY_POSITION, _lib.HISTORY_EXCLUDE, _lib.HISTORY_LATEST) == (0, 1, 2)


def _last_error(lib):
    return lib.dfm_last_error().decode()


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    """DFM_REQUIRE comes before any launch: DFM_ERR_INVALID (1) and a message, on a machine without a GPU."""
    lib = _lib.load()
    P = 0x1000                                                     # an aligned address that is never read
    build = dict(users=P, items=P, ts=P, labels=P, mask=P, order=P, start=P, n=10, n_users=3, n_items=4, pos_of=P,
                 rank=P, events=P, sorted_ts=P, event_count=P, status=P, stream=None)
    gather = dict(queries=P, m=5, mode=0, length=8, users=P, items=P, ts=P, item_ids=P, start=P, pos_of=P, rank=P,
                  events=P, sorted_ts=P, event_count=P, n=10, n_users=3, n_items=4, bag=P, count=P, gap=P, status=P,
                  stream=None)
    assert len(build) == len(_lib.SIGNATURES[NAMES[0]][1]) and len(gather) == len(_lib.SIGNATURES[NAMES[1]][1])

    def refused(fn, args, message, **change):
        assert fn(*dict(args, **change).values()) == 1, change
        assert message in _last_error(lib), (change, _last_error(lib))

    for key in ("users", "items", "ts", "order", "start", "pos_of", "rank", "events", "sorted_ts", "event_count",
                "status"):
        refused(lib.dfm_history_index_build, build, "null argument", **{key: None})
    refused(lib.dfm_history_index_build, build, "n = 2147483648 outside [0, 2^31)", n=2**31)
    refused(lib.dfm_history_index_build, build, "n = -1 outside", n=-1)
    refused(lib.dfm_history_index_build, build, "n_users = 0 outside", n_users=0)
    refused(lib.dfm_history_index_build, build, "n_items = 0 outside", n_items=0)
    refused(lib.dfm_history_index_build, build, "misaligned argument", order=P + 4)

    for key in ("queries", "users", "items", "ts", "start", "pos_of", "rank", "events", "sorted_ts", "event_count",
                "bag", "count", "gap", "status"):
        refused(lib.dfm_history_gather, gather, "null argument", **{key: None})
    for length in (0, -1, 4097):
        refused(lib.dfm_history_gather, gather, f"length = {length} outside [1, 4096]", length=length)
    refused(lib.dfm_history_gather, gather, "n = 2147483648 outside [0, 2^31)", n=2**31)
    refused(lib.dfm_history_gather, gather, "m = 2147483648 outside [0, 2^31)", m=2**31)
    refused(lib.dfm_history_gather, gather, "mode = 3", mode=3)
    refused(lib.dfm_history_gather, gather, "take more than 4294967296 bytes", m=(1 << 17) + 1, length=4096)
    refused(lib.dfm_history_gather, gather, "misaligned argument", bag=P + 4)
    # labels, the source mask and item_ids are optional, and no query is no launch
    assert lib.dfm_history_gather(*dict(gather, m=0, queries=None, bag=None).values()) == 0


# ---------------------------------------------------------------------------------------------------- training limit
def _movielens_model(length, dim=16):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.synthetic import movielens_fields, schema_from_fields
    from deepfm_amd.models import create_model
    schema = schema_from_fields(movielens_fields())
    schema.fields["hist"] = history_field("hist", length, 1682, dim)
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = 16
    cfg.dnn.hidden_units = [32, 32]
    return create_model("deepfm", schema, cfg).train()


def test_the_record_backward_admits_a_history_of_43_ids_at_width_16():
    """``16 * (256 * (d / 4 + 1) + 64 L + 1) <= 65536``: L <= 43 at d = 16, L <= 51 at d = 8."""
    from deepfm_amd.training import mixed_ineligible_reason, mixed_step_ineligible_reason
    from deepfm_amd.training.eligibility import backward_lds_bytes
    assert mixed_step_ineligible_reason(_movielens_model(20), 4096) is None
    at_cap = _movielens_model(43)
    assert mixed_step_ineligible_reason(at_cap, 4096) is None
    assert backward_lds_bytes(at_cap) == 16 * (256 * 5 + 64 * 43 + 1) <= _lib.BWD_RECORD_LDS_BYTES
    over = _movielens_model(44)
    reason = mixed_step_ineligible_reason(over, 4096)
    assert reason is not None and "bytes of LDS for the widest field, over its cap of 65536" in reason
    assert mixed_ineligible_reason(over) is None                   # the predictors have no such limit
    assert mixed_step_ineligible_reason(_movielens_model(51, dim=8), 4096) is None
    assert "over its cap of 65536" in mixed_step_ineligible_reason(_movielens_model(52, dim=8), 4096)
