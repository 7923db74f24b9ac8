"""GPU: history bags formed at record assembly (``dfm_assemble_plan_bind_history``, ``HistoryBag``; DESIGN.md §7b
"History bags at record assembly").  The criterion everywhere is equality of bytes: a record assembled from a column
bound to the history index equals the record the same loader writes when that column is the materialised tensor
``bag.materialize().bag``.  No tolerance is involved, and every launch over a bound column is issued twice.

1. the matrix: the logs of ``tests/test_gpu_history.py`` (segments of 0, 1, 63, 64, 65, 129 and 200 rows, a user at
   one timestamp, a user without an event), lengths that divide a wavefront, do not, and exceed it, every ``ties``,
   index option, batch size around the wavefront and workgroup edges, shuffle, and the four plan shapes;
2. 140 000 bags of 4096 ids (4.6 GB) that ``materialize()`` refuses are served from under 64 MB;
3. the refusals, and a bad ``order`` entry;
4. end to end: a fused training step, ``evaluate_loader`` and the int8 predictor over both loaders.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.test_gpu_history import DEV, N_ITEMS, SEGMENTS, _dev, _np, make_log

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 8, 64, 65, 200)          # 3 does not divide 64; 65 and 200 are wider than a wavefront
BATCHES = (1, 63, 64, 65, 257)            # the wavefront and workgroup edges inside, on and past a batch
PLANS = ("plain", "negatives", "ragged", "tail")
K = 2
MIN_ROWS = 300                            # rows of the columns: above the largest batch


def _schema(n_users, L, dim=8):
    from deepfm_amd.data import history_field
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    return DatasetSchema(fields={
        "user_id": FieldSchema("user_id", FeatureType.SPARSE, n_users + 1, dim, "user"),
        "item_id": FieldSchema("item_id", FeatureType.SPARSE, N_ITEMS + 1, dim, "item"),
        "hist": history_field("hist", L, 500, dim)})                  # ids of the item_ids maps below stay under 500


def _seen(n_users, short):
    """Seen-sets that do not depend on the log: everybody has seen item 0 alone; with ``short`` user 0 has one unseen
    row left, fewer than K, so a truncating source over it is ragged."""
    from deepfm_amd.data import SeenSets
    u, i = np.arange(n_users, dtype=np.int64), np.zeros(n_users, np.int64)
    if short:
        u = np.concatenate([u, np.zeros(N_ITEMS - 2, np.int64)])
        i = np.concatenate([i, np.arange(1, N_ITEMS - 1, dtype=np.int64)])
    return SeenSets.from_interactions(u, i, n_users, N_ITEMS)


def _loader(schema, ids, labels, bag, user_of, plan, batch, shuffle, seed=5, roles=None, table_extra=None):
    """A loader over (ids, labels, bag), ``bag`` a tensor or a ``HistoryBag``, in one of the four plan shapes."""
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, ItemTable, NegativeSampler
    dense = torch.empty(0, ids.shape[1], dtype=torch.float32, device=DEV)
    cols = DeviceColumns.from_device(schema, ids, dense, labels, bags=[bag])
    sampler = None
    if plan in ("negatives", "ragged"):
        n_users = schema.fields["user_id"].vocabulary_size - 1
        table = ItemTable(schema, dict({"item_id": np.arange(N_ITEMS, dtype=np.int64) + 1}, **(table_extra or {})))
        sampler = NegativeSampler(cols, _seen(n_users, plan == "ragged"), user_of, table, K, seed=3, roles=roles,
                                  short_users="truncate" if plan == "ragged" else "refuse")
        assert (sampler.counts is not None) == (plan == "ragged" and 0 in user_of)
    return DeviceEpochLoader(cols, batch, shuffle=shuffle, seed=seed, negatives=sampler, depth=2)


def _hist_block(loader, rec, lay=None):
    lay = lay or loader.layout
    return lay.views(rec)[3][0]


def _compare(bound, plain, plan):
    """Every record of interest of the two loaders, bit for bit; the bound one twice.  Returns the launches compared."""
    assert bound.rows == plain.rows and bound.num_batches == plain.num_batches and bound.tail_rows == plain.tail_rows
    B, launches = bound.batch_size, 0
    for loader in (bound, plain):
        loader.set_epoch(1)
    if bound.shuffle:
        assert torch.equal(bound.order, plain.order)
    for k in sorted({0, bound.num_batches // 2, bound.num_batches - 1}):
        first, again, want = bound.record(k).clone(), bound.record(k), plain.record(k)
        assert torch.equal(first, again) and torch.equal(first, want), (plan, "batch", k)
        launches += 1
    if plan == "tail":
        assert bound.tail_rows > 0
    if bound.tail_rows:
        first, again, want = bound.tail().clone(), bound.tail(), plain.tail()
        assert torch.equal(first, again) and torch.equal(first, want), (plan, "tail")
        launches += 1
    # fewer rows than slots: the padding slots' bags are all zero
    count, start = B // 2, bound.rows - B // 2
    first, again = bound.rows_into_next(start, count).clone(), bound.rows_into_next(start, count)
    assert torch.equal(first, again) and torch.equal(first, plain.rows_into_next(start, count)), (plan, "padding")
    block = _hist_block(bound, first)
    assert block.shape == (B, bound.layout.seq_lengths[0]) and not bool(block[count:].any())
    return launches + 1


# ----------------------------------------------------------------------------- 1. the matrix
@pytest.mark.parametrize("n_users", [1, 3, 70])
def test_a_bound_column_gives_the_bytes_of_the_materialised_one(n_users):
    from deepfm_amd.data import HistoryBag
    rng = np.random.default_rng(100 + n_users)
    seen = dict(cut=False, shorter=False, empty=False, full=False, ragged=False, repeats=False)
    combos, variation, k2, launches = set(), 0, 0, 0
    for segments in SEGMENTS[n_users]:
        log, host, _ = make_log(segments, rng)
        n = len(log)
        ids_map = rng.integers(1, 500, N_ITEMS).astype(np.int64)
        ids_map[[5, 17]] = 0                                        # two items share the padding id
        half = _dev(rng.permutation(n)[:n // 2].astype(np.int64))
        for source, item_ids in itertools.product((None, half), (None, ids_map)):
            index = log.history_index(source, True, None if item_ids is None else _dev(item_ids))
            variation += 1
            for t, ties in enumerate(("position", "exclude", "latest")):
                if n == 0 and ties != "latest":
                    continue                                        # an empty log has no row to ask about
                limit = n_users if ties == "latest" else n
                q = np.concatenate([np.arange(limit), rng.integers(0, limit, max(MIN_ROWS - limit, limit // 4))])
                q = q[rng.permutation(len(q))].astype(np.int64)     # every row once, then repeats, shuffled
                seen["repeats"] |= len(np.unique(q)) < len(q)
                m, L = len(q), LENGTHS[(variation + 2 * t) % len(LENGTHS)]      # six variations: every (L, ties)
                bag = HistoryBag(index, _dev(q), L, ties=ties)
                assert len(bag) == m and bag.length == L
                whole = bag.materialize()
                count = _np(whole.count)
                seen["cut"] |= bool((count > L).any())
                seen["full"] |= bool((count >= L).any())
                seen["shorter"] |= bool(((count > 0) & (count < L)).any())
                seen["empty"] |= bool((count == 0).any())
                user_of = (q if ties == "latest" else host[0][q]).astype(np.int32)
                ids = torch.stack([_dev(user_of.astype(np.int64) + 1),
                                   _dev(rng.integers(1, N_ITEMS + 1, m).astype(np.int64))]).contiguous()
                labels = _dev((rng.random(m) < 0.5).astype(np.float32))
                schema = _schema(n_users, L)
                for plan in PLANS:
                    if n == 0 and plan in ("negatives", "ragged"):
                        continue
                    batch, shuffle = BATCHES[k2 % len(BATCHES)], bool((k2 // 20) % 2)
                    k2 += 1
                    rows = m * (1 + K) if plan == "negatives" else m
                    if plan == "tail" and rows % batch == 0:
                        batch = 63                                  # rows is no multiple of both 63 and 64 ...
                        batch = 64 if rows % batch == 0 else batch
                    pair = [_loader(schema, ids, labels, b, user_of, plan, batch, shuffle) for b in (bag, whole.bag)]
                    seen["ragged"] |= pair[0].negatives is not None and pair[0].negatives.counts is not None
                    launches += _compare(*pair, plan)
                    combos.add((plan, batch, shuffle))
                    combos.add(("L", L, ties))
    # what the matrix covered: a bag cut by L, one shorter than L, an empty one; every plan at every batch size, both
    # orders; every length under every tie rule
    assert seen == dict.fromkeys(seen, True), seen
    assert {(p, b) for p, b, _ in combos if p in PLANS[:3]} == set(itertools.product(PLANS[:3], BATCHES))
    assert {s for p, _, s in combos if p in PLANS} == {False, True}
    if n_users == 1:
        assert {(l, t) for p, l, t in combos if p == "L"} == set(itertools.product(LENGTHS, ("position", "exclude",
                                                                                               "latest")))
    assert launches >= 4 * len(PLANS) * 3


# ----------------------------------------------------------------------------- 2. the 4 GiB cap
def test_bags_that_cannot_be_materialised_are_served_from_the_index():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, DeviceInteractionLog, HistoryBag
    from deepfm_amd.data.packed import PackedColumns
    rng = np.random.default_rng(2)
    n, n_users, m, L, B = 1000, 3, 140_000, 4096, 64
    user = rng.integers(0, n_users, n).astype(np.int64)
    item = rng.integers(0, N_ITEMS, n).astype(np.int64)
    ts = rng.integers(0, 50, n).astype(np.int64)
    log = DeviceInteractionLog(user, item, ts, np.ones(n, np.float32), n_users, N_ITEMS, DEV)
    index = log.history_index()
    q = rng.integers(0, n, m).astype(np.int64)
    schema = _schema(n_users, L)
    ids = torch.stack([_dev(user[q] + 1), _dev(item[q] + 1)]).contiguous()
    labels = _dev((rng.random(m) < 0.5).astype(np.float32))
    dense = torch.empty(0, m, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    queries = _dev(q)
    bag = HistoryBag(index, queries, L)
    cols = DeviceColumns.from_device(schema, ids, dense, labels, bags=[bag])
    loader = DeviceEpochLoader(cols, B, shuffle=True, seed=1, depth=4)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    print(f"memory_allocated grew by {grown} bytes; the bags would take {m * L * 8}")
    assert m * L * 8 > 4.5e9 and grown < 64 * 2**20
    with pytest.raises(ValueError, match=f"{m} bags of {L} ids take {m * L * 8} bytes, more than 4294967296"):
        bag.materialize()
    rec = loader.record(0)
    assert torch.equal(rec, loader.record(0))
    rows = loader.order[:B]
    want_bag = index.lookup(queries[rows], L).bag
    assert bool((want_bag[:, 200] != 0).any()) and not bool(want_bag[:, 400:].any())     # ~333 events per user
    r = _np(rows)
    host = PackedColumns(schema, {"user_id": user[q][r] + 1, "item_id": item[q][r] + 1, "hist": _np(want_bag)},
                         _np(labels)[r])
    want = np.zeros(loader.layout.record_bytes, np.uint8)
    loader.layout.write(want, host, 0, B)
    assert np.array_equal(_np(rec), want)


# ----------------------------------------------------------------------------- 3. refusals and padding
def _small(L=6, m=MIN_ROWS):
    from deepfm_amd.data import HistoryBag
    rng = np.random.default_rng(9)
    log, host, _ = make_log((65, 0, 200), rng)
    index = log.history_index()
    q = rng.integers(0, len(log), m).astype(np.int64)
    bag = HistoryBag(index, _dev(q), L)
    user_of = host[0][q].astype(np.int32)
    ids = torch.stack([_dev(user_of.astype(np.int64) + 1), _dev(rng.integers(1, N_ITEMS + 1, m).astype(np.int64))])
    return log, index, q, bag, user_of, ids.contiguous(), _dev((rng.random(m) < 0.5).astype(np.float32))


def test_refusals_name_the_field_and_come_before_any_launch():
    from deepfm_amd.data import DeviceColumns, HistoryBag, Role
    L = 6
    log, index, q, bag, user_of, ids, labels = _small(L)
    n, m, schema = len(log), len(q), _schema(3, L)
    item_bags = {"hist": np.zeros((N_ITEMS, L), np.int64)}
    with pytest.raises(ValueError, match="field 'hist' is a HistoryBag with role ITEM"):
        _loader(schema, ids, labels, bag, user_of, "negatives", 64, False, roles={"hist": Role.ITEM},
                table_extra=item_bags)
    dense = torch.empty(0, m, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match=f"bag of 'hist': expected a HistoryBag of {m} queries and length {L} on "
                                         f"cuda:0, got {m - 1} queries"):
        DeviceColumns.from_device(schema, ids, dense, labels, bags=[HistoryBag(index, bag.queries[1:], L)])
    with pytest.raises(ValueError, match=f"expected a HistoryBag of {m} queries and length {L} on cuda:0, got {m} "
                                         f"queries and length {L + 1}"):
        DeviceColumns.from_device(schema, ids, dense, labels, bags=[HistoryBag(index, bag.queries, L + 1)])
    with pytest.raises(ValueError, match=f"2 of 4 entries of queries are outside the log's {n} rows"):
        HistoryBag(index, _dev(np.array([0, n, 3, -1], np.int64)), L, ties="exclude")
    with pytest.raises(ValueError, match="1 of 3 entries of queries are outside the user table's 3 rows"):
        HistoryBag(index, _dev(np.array([2, 3, 0], np.int64)), L, ties="latest")
    assert len(HistoryBag(index, _dev(np.array([2, 1, 0], np.int64)), L, ties="latest")) == 3


def test_the_entry_point_refuses_a_bad_column_kind_role_or_mode_and_the_plan_stays_as_it_was():
    from deepfm_amd import _lib
    from deepfm_amd.data import Role
    L = 6
    log, index, q, bag, user_of, ids, labels = _small(L)
    schema = _schema(3, L)
    whole = bag.materialize().bag
    bound, plain = (_loader(schema, ids, labels, b, user_of, "negatives", 64, True) for b in (bag, whole))
    lib = _lib.load()

    def refused(loader, column, message, **change):
        src = bag.source()
        for key, value in change.items():
            setattr(src, key, value)
        assert lib.dfm_assemble_plan_bind_history(loader._plan, column, src) == 1, (column, change)
        assert message in lib.dfm_last_error().decode(), lib.dfm_last_error().decode()

    refused(bound, -1, "column -1 outside [0, 3)")
    refused(bound, 3, "column 3 outside [0, 3)")
    refused(bound, 0, "column 0: only a SEQUENCE column is bound")
    for mode in (-1, 3):
        refused(bound, 2, f"mode = {mode}: expected DFM_HISTORY_POSITION", mode=mode)
    refused(bound, 2, "n = 2147483648 outside [0, 2^31)", n=2**31)
    refused(bound, 2, "n_users = 0 outside [1, 2^31)", n_users=0)
    refused(bound, 2, "n_items = -1 outside [1, 2^31)", n_items=-1)
    refused(bound, 2, "null argument", d_start=None)
    refused(bound, 2, "null argument", d_events=None)
    refused(bound, 2, "misaligned argument", d_rank=index.rank.data_ptr() + 2)
    assert lib.dfm_assemble_plan_bind_history(None, 2, bag.source()) == 1
    assert lib.dfm_assemble_plan_bind_history(bound._plan, 2, None) == 1
    # a tensor column whose role is ITEM: the plan exists, and binding it is refused for its role
    item_role = _loader(schema, ids, labels, whole, user_of, "negatives", 64, False, roles={"hist": Role.ITEM},
                        table_extra={"hist": np.zeros((N_ITEMS, L), np.int64)})
    refused(item_role, 2, "column 2: role 1: a history is its positive's (DFM_ROLE_COPY)")
    # nothing of that changed a plan: the refused loader still writes its ITEM bags, the bound one its histories
    item_role.set_epoch(1)
    last = item_role.record(item_role.num_batches - 1)
    assert not bool(_hist_block(item_role, last).any())             # negatives: rows of the all-zero item table
    assert _compare(bound, plain, "negatives") >= 3
    # binding again re-points the column: to the "latest" rule over user rows, and back
    users = _dev(user_of.astype(np.int64))
    src = bag.source()
    src.mode = _lib.HISTORY_LATEST
    pos = bound.columns.bags[0].queries
    saved = pos.clone()
    pos.copy_(users)
    assert lib.dfm_assemble_plan_bind_history(bound._plan, 2, src) == 0
    latest = index.latest(users, L).bag
    other = _loader(schema, ids, labels, latest, user_of, "negatives", 64, True)
    for loader in (bound, other):
        loader.set_epoch(1)
    assert torch.equal(bound.record(1), other.record(1)) and not torch.equal(bound.record(1), plain.record(1))
    pos.copy_(saved)
    assert lib.dfm_assemble_plan_bind_history(bound._plan, 2, bag.source()) == 0
    assert torch.equal(bound.record(1), plain.record(1))


@pytest.mark.parametrize("plan", ["negatives", "ragged"])
def test_a_bad_order_entry_is_an_all_zero_bag_and_zero_ids(plan):
    L = 6
    log, index, q, bag, user_of, ids, labels = _small(L)
    schema = _schema(3, L)
    bound, plain = (_loader(schema, ids, labels, b, user_of, plan, 65, True) for b in (bag, bag.materialize().bag))
    for loader in (bound, plain):
        loader.set_epoch(2)
        loader.order[[0, 64, 70]] = torch.tensor([-1, loader.rows, 2**40], device=DEV)
    got, want = bound.record(0), plain.record(0)
    assert torch.equal(got, want) and torch.equal(bound.record(1), plain.record(1))
    ids_blk, _, labels_blk, bags = bound.layout.views(got)
    for slot in (0, 64):
        assert not bool(ids_blk[:, slot].any()) and not bool(bags[0][slot].any()) and float(labels_blk[slot]) == 0.0
    assert bool(bags[0][1:64].any()) and bool(ids_blk[:, 1:64].all())


# ----------------------------------------------------------------------------- 4. end to end
def test_a_bound_bag_trains_evaluates_and_serves_like_the_materialised_one():
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data import (DeviceColumns, DeviceEpochLoader, DeviceInteractionLog, HistoryBag, ItemTable,
                                 NegativeSampler, Role, history_field)
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    from deepfm_amd.models import create_model
    from deepfm_amd.training import (DenseTableAdam, FusedMixedDeepFMStep, MixedSchemaPredictor,
                                     QuantizedMixedPredictor)
    rng = np.random.default_rng(8)
    n, n_users, n_items, L, B = 600, 12, 40, 5, 64
    user = rng.integers(0, n_users, n).astype(np.int64)
    item = rng.integers(0, n_items, n).astype(np.int64)
    ts = rng.integers(0, 60, n).astype(np.int64)
    labels = (rng.random(n) < 0.6).astype(np.float32)
    log = DeviceInteractionLog(user, item, ts, labels, n_users, n_items, DEV)
    split = log.leave_one_out_split(3)
    schema = DatasetSchema(fields={
        "user_id": FieldSchema("user_id", FeatureType.SPARSE, n_users + 1, 16, "user"),
        "item_id": FieldSchema("item_id", FeatureType.SPARSE, n_items + 1, 16, "item"),
        "hist": history_field("hist", L, n_items, 16)})
    rows = split.train
    bag = HistoryBag(log.history_index(source=rows), rows, L)
    whole = bag.materialize().bag
    assert bool((whole != 0).any()) and not bool(whole[:, L - 1].all()) and bool(whole[:, L - 1].any())
    ids = torch.stack([log.user_rows[rows] + 1, log.item_rows[rows] + 1]).contiguous()
    dense = torch.empty(0, len(rows), dtype=torch.float32, device=DEV)
    table = ItemTable(schema, {"item_id": np.arange(n_items, dtype=np.int64) + 1})
    loaders = []
    for b in (bag, whole):
        dcols = DeviceColumns.from_device(schema, ids, dense, log.labels[rows].contiguous(), bags=[b])
        sampler = NegativeSampler(dcols, log.seen_sets(), _np(log.user_rows[rows]).astype(np.int32), table, K, seed=6)
        assert sampler.roles == {"user_id": Role.COPY, "item_id": Role.ITEM, "hist": Role.COPY}
        loaders.append(DeviceEpochLoader(dcols, B, shuffle=True, seed=2, negatives=sampler, depth=2))
        loaders[-1].set_epoch(1)
    assert loaders[0].columns.field_columns()["hist"] is bag and len(loaders[0]) >= 3

    def make():
        cfg = ExperimentConfig()
        cfg.feature.fm_embed_dim = 16
        cfg.dnn.hidden_units, cfg.dnn.dropout = [32, 32], 0.1
        torch.manual_seed(3)
        model = create_model("deepfm", schema, cfg).cuda().train()
        model.embedding.strict_indices = True
        return model

    results = []
    for loader in loaders:
        model = make()
        opt = DenseTableAdam(model, lr=1e-2, l2=1e-3, max_grad_norm=0.5)
        step = FusedMixedDeepFMStep(model, opt, B, use_graph=True)
        step.capture()
        got = []
        for k in (0, len(loader) - 1):
            step.run_from(loader.record(k))
            model.embedding.raise_on_bad_index()
            got.append(step.loss.clone())
        torch.cuda.synchronize()
        got.append(opt.flat_param.clone())
        pred = MixedSchemaPredictor(model, B)
        metrics = pred.evaluate_loader(loader, ranking_ks=[1, 5], group_auc=True)
        quant = QuantizedMixedPredictor(model, B, fmt="int8")
        assert "hist" in quant.tables.records
        got.append(quant.predict_from(loader.record(0)).clone())
        torch.cuda.synchronize()
        results.append((got, metrics))
    (a, ma), (b, mb) = results
    assert len(a) == len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(bool(torch.isfinite(x).all()) for x in a)
    assert list(ma) == list(mb) and {"auc", "logloss", "HR@5", "gauc"} <= set(ma) and ma == mb
