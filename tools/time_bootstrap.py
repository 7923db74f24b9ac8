#!/usr/bin/env python3
"""Time of the Poisson bootstrap (``training/metrics.py:compute_bootstrap``, csrc/bootstrap.hip), three cases:
  * ``compute_bootstrap`` on 1 M samples, 200 replicates, every sample its own unit (device tensors in, dict out on the
    host): wall clock of whole calls, the device time of the bootstrap's own launches (prepare, two ``torch.sort``,
    replicates) by device events over back-to-back calls, and of the replicate passes alone (the sorted keys kept);
    beside each time the element visits per second, 2 n R per call (every replicate meets every sample in both orders);
  * the same with 10 K user units;
  * each against a host loop of ``roc_auc_score(sample_weight=w)`` + ``log_loss(sample_weight=w)`` with numpy Poisson
    weights, the copy of labels and scores to the host included.  The host loop is timed at ``--host-replicates``
    (5) replicates and scaled to 200: it is linear in them;
  * ``evaluate_loader(..., bootstrap=200, bootstrap_by="user_id")`` against the same call without the keywords, on the
    MovieLens schema (DeepFM of configs/deepfm_movielens.yaml, B = 4096) over 943 users x 1000 candidates, alternating.
Medians and ranges over ``--reps`` repetitions; one JSON line per case.

``--grouped`` times the bootstrap of the per-user metrics instead (``compute_bootstrap_ranking``,
csrc/bootstrap_units.hip), ks = [1, 5, 10, 20] with gauc / uauc, 200 replicates, at 943 users x 1000 candidates and at
10^6 users x 10 candidates: whole calls; the ``dfm_bootstrap_units`` launches alone over columns formed once, beside
their byte floor (columns x users x 8 bytes per replicate block at 8 TB/s, plus an empty launch); a host loop of the
numpy restatement's weighted sums and quotients over the same columns (``tests/bootstrap_units_reference.py``), timed at
``--host-replicates`` and scaled to 200; and ``evaluate_loader(..., bootstrap_grouped=True)`` against the same call
without the keyword (943 x 1000).
usage: python tools/time_bootstrap.py [--reps 15] [--host-replicates 5] [--grouped]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_gauc import stats, wall  # noqa: E402
from tools.time_predict_mixed import B, C, U, build, split  # noqa: E402

REPLICATES = 200


def device_ms(fn, reps, calls=5):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)                         # ms
    return out


def visits_per_s(n, ms):
    return round(2.0 * n * REPLICATES / (float(np.median(ms)) * 1e-3), 0)


def replicate_passes(y, s, uid):
    """The second call alone, over keys that were prepared and sorted once."""
    from deepfm_amd import _lib
    lib = _lib.load()
    n = s.numel()
    keys = torch.empty(2, n, dtype=torch.int64, device=s.device)
    ws = torch.empty(lib.dfm_bootstrap_workspace_bytes(n, REPLICATES), dtype=torch.uint8, device=s.device)
    _lib.check(lib.dfm_bootstrap_prepare(y.data_ptr(), s.data_ptr(), _lib.ptr(uid), n, keys[0].data_ptr(),
                                         keys[1].data_ptr(), ws.data_ptr(), _lib.stream_handle()))
    ordered = torch.sort(keys, dim=1).values
    counts = torch.empty(REPLICATES, 5, dtype=torch.int64, device=s.device)
    values = torch.empty(REPLICATES, 2, dtype=torch.float64, device=s.device)
    faults = torch.empty(3, dtype=torch.int64, device=s.device)

    def run():
        _lib.check(lib.dfm_bootstrap_replicates(ordered[0].data_ptr(), ordered[1].data_ptr(), _lib.ptr(uid), n,
                                                REPLICATES, 0, ws.data_ptr(), counts.data_ptr(), values.data_ptr(),
                                                faults.data_ptr(), _lib.stream_handle()))
    return run


def large_case(reps, host_replicates, units):
    from sklearn.metrics import log_loss, roc_auc_score
    from deepfm_amd.training import bootstrap_device, compute_bootstrap
    n = 1_000_000
    rng = np.random.default_rng(1)
    y = (rng.random(n) < 0.3).astype(np.float32)
    s = (rng.random(n) * 0.5 + 0.2 * y).astype(np.float32)
    u = rng.integers(0, units, n) if units else None
    d_y, d_s = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
    d_u = torch.from_numpy(u).cuda() if units else None
    for _ in range(3):
        got = compute_bootstrap(d_y, d_s, REPLICATES, unit_ids=d_u)
    whole = [wall(lambda: compute_bootstrap(d_y, d_s, REPLICATES, unit_ids=d_u))[0] for _ in range(reps)]
    launches = device_ms(lambda: bootstrap_device(d_y, d_s, REPLICATES, 0, d_u), reps)
    passes = device_ms(replicate_passes(d_y, d_s, d_u), reps)

    def host_loop():
        hy, hs = d_y.cpu().numpy(), d_s.cpu().numpy().astype(np.float64)
        hu = d_u.cpu().numpy() if units else None
        gen = np.random.default_rng(0)
        out = []
        for _ in range(host_replicates):
            w = gen.poisson(1.0, units or n)
            w = w[hu] if units else w
            out.append((roc_auc_score(hy, hs, sample_weight=w), log_loss(hy, hs, sample_weight=w)))
        return np.array(out)

    host = []
    for _ in range(3):
        t, ref = wall(host_loop)
        host.append(t * REPLICATES / host_replicates)
    print(json.dumps(dict(case="compute_bootstrap", samples=n, units=units or n, replicates=REPLICATES, reps=reps,
                          whole_call_ms=stats(whole), whole_call_visits_per_s=visits_per_s(n, np.asarray(whole) * 1e3),
                          device_ms=stats(launches, scale=1.0), device_visits_per_s=visits_per_s(n, launches),
                          replicate_passes_ms=stats(passes, scale=1.0),
                          replicate_passes_visits_per_s=visits_per_s(n, passes),
                          host_loop_s_scaled_to_200=stats(host, scale=1.0), host_replicates_timed=host_replicates,
                          auc=got["auc"], auc_se=got["auc_se"], auc_se_host=float(np.std(ref[:, 0], ddof=1)),
                          logloss_se=got["logloss_se"], logloss_se_host=float(np.std(ref[:, 1], ddof=1)))), flush=True)


def evaluation_case(reps):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import MixedSchemaPredictor
    rng = np.random.default_rng(0)
    model = build("deepfm")
    feats, labels = split(rng)
    loader = DeviceEpochLoader(DeviceColumns(PackedColumns(model.schema, feats, labels), "cuda"), B, shuffle=False)
    pred = MixedSchemaPredictor(model, B)
    kw = dict(bootstrap=REPLICATES, bootstrap_by="user_id")
    for on in (False, True, False, True):                         # warm-up of both forms
        m = pred.evaluate_loader(loader, **(kw if on else {}))
    plain, boot = [], []
    for _ in range(reps):                                         # alternating: the same neighbours for both
        plain.append(wall(lambda: pred.evaluate_loader(loader))[0])
        boot.append(wall(lambda: pred.evaluate_loader(loader, **kw))[0])
    print(json.dumps(dict(case="evaluate_loader", split=f"{U}x{C}", B=B, replicates=REPLICATES, reps=reps,
                          without_ms=stats(plain), with_ms=stats(boot),
                          difference_of_medians_ms=round(float(np.median(boot) - np.median(plain)) * 1e3, 3),
                          auc=m["auc"], auc_se=m["auc_se"], auc_lo=m["auc_lo"], auc_hi=m["auc_hi"])), flush=True)


KS = [1, 5, 10, 20]
HBM_BYTES_PER_S = 8e12


def grouped_case(reps, host_replicates, users, cands):
    from deepfm_amd import _lib
    from deepfm_amd.training import bootstrap_units_device, compute_bootstrap_ranking
    from deepfm_amd.training import metrics as M
    from tests import bootstrap_units_reference as UR
    n = users * cands
    rng = np.random.default_rng(1)
    u = np.repeat(np.arange(users, dtype=np.int64), cands)
    y = np.zeros(n, np.float32)
    y[np.arange(users) * cands + rng.integers(0, cands, users)] = 1.0
    s = (rng.random(n) * 0.5 + 0.2 * y).astype(np.float32)
    d_u, d_y, d_s = (torch.from_numpy(a).cuda() for a in (u, y, s))
    call = lambda: compute_bootstrap_ranking(d_u, d_y, d_s, KS, REPLICATES, 0, users, True)      # noqa: E731
    for _ in range(3):
        got = call()
    whole = [wall(call)[0] for _ in range(reps)]
    # the columns once, as bootstrap_grouped_device forms them: 1 + 2 len(KS) of the ranks, 4 of the groups
    lib = _lib.load()
    cols = torch.empty(1 + 2 * len(KS) + 4, users, dtype=torch.int64, device="cuda")
    rank, _ = M.ranking_user_ranks_device(d_u, d_y, d_s, users)
    gain = M._gain_table(KS, d_s.device)
    import ctypes
    _lib.check(lib.dfm_bootstrap_rank_columns(rank.data_ptr(), users, (ctypes.c_int32 * len(KS))(*KS), len(KS),
                                              gain.data_ptr(), gain.numel(), cols.data_ptr(), _lib.stream_handle()))
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.dfm_grouped_auc_workspace_bytes(n, users), dtype=torch.uint8, device="cuda")
    _lib.check(lib.dfm_grouped_auc_prepare(d_u.data_ptr(), d_y.data_ptr(), d_s.data_ptr(), n, users, keys.data_ptr(),
                                           ws.data_ptr(), _lib.stream_handle()))
    ordered = torch.sort(keys).values
    _lib.check(lib.dfm_grouped_auc_unit_columns(ordered.data_ptr(), n, users, ws.data_ptr(),
                                                cols[1 + 2 * len(KS):].data_ptr(), _lib.stream_handle()))
    units = device_ms(lambda: bootstrap_units_device(cols, REPLICATES, 0), reps, calls=20)
    empty = device_ms(lambda: lib.dfm_debug_empty_launch(_lib.stream_handle()), reps, calls=20)
    blocks = -(-REPLICATES // _lib.BOOTSTRAP_REPLICATE_BLOCK)
    floor_ms = cols.shape[0] * users * 8 * blocks / HBM_BYTES_PER_S * 1e3 + float(np.median(empty))
    host_cols = cols.cpu().numpy()

    def host_loop():
        return UR.replicate_values(UR.weighted_sums(host_cols, host_replicates, 0), len(KS), True)

    host = [wall(host_loop)[0] * REPLICATES / host_replicates for _ in range(3)]
    print(json.dumps(dict(case="compute_bootstrap_ranking", users=users, candidates=cands, ks=KS, group_auc=True,
                          columns=int(cols.shape[0]), replicates=REPLICATES, reps=reps, whole_call_ms=stats(whole),
                          units_launches_ms=stats(units, scale=1.0, digits=4),
                          empty_launch_ms=stats(empty, scale=1.0, digits=4), units_byte_floor_ms=round(floor_ms, 4),
                          host_loop_s_scaled_to_200=stats(host, scale=1.0), host_replicates_timed=host_replicates,
                          **{k: got[k] for k in ("HR@10", "HR@10_se", "HR@10_lo", "HR@10_hi", "NDCG@10_se", "gauc",
                                                 "gauc_se")})), flush=True)


def grouped_evaluation_case(reps):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import MixedSchemaPredictor
    rng = np.random.default_rng(0)
    model = build("deepfm")
    feats, labels = split(rng)
    loader = DeviceEpochLoader(DeviceColumns(PackedColumns(model.schema, feats, labels), "cuda"), B, shuffle=False)
    pred = MixedSchemaPredictor(model, B)
    kw = dict(ranking_ks=KS, group_auc=True, bootstrap=REPLICATES, bootstrap_by="user_id")
    for on in (False, True, False, True):                         # warm-up of both forms
        m = pred.evaluate_loader(loader, bootstrap_grouped=on, **kw)
    plain, grouped = [], []
    for _ in range(reps):                                         # alternating: the same neighbours for both
        plain.append(wall(lambda: pred.evaluate_loader(loader, **kw))[0])
        grouped.append(wall(lambda: pred.evaluate_loader(loader, bootstrap_grouped=True, **kw))[0])
    print(json.dumps(dict(case="evaluate_loader_grouped", split=f"{U}x{C}", B=B, replicates=REPLICATES, reps=reps,
                          without_ms=stats(plain), with_ms=stats(grouped),
                          difference_of_medians_ms=round(float(np.median(grouped) - np.median(plain)) * 1e3, 3),
                          **{k: m[k] for k in ("HR@10", "HR@10_se", "HR@10_lo", "HR@10_hi", "gauc", "gauc_se")})),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-replicates", type=int, default=5)
    ap.add_argument("--only", choices=["evaluate_loader", "compute_bootstrap"], default=None)
    ap.add_argument("--grouped", action="store_true", help="the per-user metrics (compute_bootstrap_ranking)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bootstrap.py measures on the device: no GPU found")
    if args.grouped:
        if args.only != "evaluate_loader":
            grouped_case(args.reps, args.host_replicates, U, C)
            grouped_case(args.reps, args.host_replicates, 1_000_000, 10)
        if args.only != "compute_bootstrap":
            grouped_evaluation_case(args.reps)
        return
    if args.only != "evaluate_loader":
        large_case(args.reps, args.host_replicates, 0)
        large_case(args.reps, args.host_replicates, 10_000)
    if args.only != "compute_bootstrap":
        evaluation_case(args.reps)


if __name__ == "__main__":
    main()
