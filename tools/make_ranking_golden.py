#!/usr/bin/env python3
"""HR@k / NDCG@k of the REFERENCE on synthetic leave-one-out splits -> tests/golden/ranking_reference.npz.

Needs a checkout of the reference (it is imported, not copied), as tools/make_golden.py does.  The reference's own
code computes every expected value: ``Trainer._compute_ranking_metrics`` (trainer.py:296-332, users with both
classes) called unbound on a stand-in ``self`` that carries ``ranking_evaluator = RankingEvaluator(ks)`` and a
stand-in dataset with ``features["user_id"]``, and ``RankingEvaluator.evaluate`` (metrics.py:62-111) on the
per-user lists of every user (the unfiltered form).  ``deepfm.config`` imports ``dacite``, which is not
installed and not needed here: a stand-in with ``from_dict = None`` takes its place in ``sys.modules``.

Scores are small integer codes times a power of two (``code * scale``, ``scale`` = 2^-7, 2^-6 or 2^-5), distinct
within each user (asserted), so that the reference's unstable ``np.argsort(-s)`` has no ties to order and every score is
exact in float32.  The fixture is kept small by storing codes, not floats:

``<c>/user_ids`` (int64), ``<c>/labels`` (uint8), ``<c>/score_codes`` (uint8) and ``<c>/score_scale`` hold a case's
samples; a case with ``<c>/base`` instead takes the samples of case ``base`` reordered by the stride permutation
``sample j <- base sample (j * <c>/stride) mod n`` (``stride`` coprime to ``n``: consecutive samples belong to different
users).  ``<c>/ks`` (int32), ``<c>/trainer`` and ``<c>/evaluator`` (the reference's dicts as JSON strings, key order
kept) are stored for every case; ``cases`` lists the case names.  ``tests/test_cpu_ranking.py:load_case`` decodes a
case.  Loads with ``allow_pickle=False``.

usage: python tools/make_ranking_golden.py REFERENCE_CHECKOUT   (the directory holding the reference's deepfm/)
"""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(ref):
    sys.path.insert(0, ref)
    sys.modules.setdefault("dacite", types.SimpleNamespace(from_dict=None))
    from deepfm.training.metrics import RankingEvaluator
    from deepfm.training.trainer import Trainer
    return Trainer, RankingEvaluator


def _codes(rng, lengths, levels=128):
    """Per user: distinct codes out of ``levels`` (uint8)."""
    return np.concatenate([rng.choice(levels, size=m, replace=False) for m in lengths]).astype(np.uint8)


def _loo(rng, users, cands):
    """``users`` users with 1 positive + (cands - 1) negatives each, contiguous, the positive at a random slot."""
    uid = np.repeat(np.arange(users, dtype=np.int64), cands)
    lab = np.zeros(users * cands, np.uint8)
    lab[np.arange(users) * cands + rng.integers(0, cands, users)] = 1
    return uid, lab, _codes(rng, [cands] * users)


def _mixed(rng):
    """Several positives, all-negative, all-positive, short (< max k) and single-sample users, interleaved."""
    uids, labs, lengths = [], [], []
    for u in range(600):
        kind = u % 6
        m = {0: 30, 1: 25, 2: 12, 3: 7, 4: 1, 5: 3}[kind] + int(rng.integers(0, 5))
        if kind == 4:
            m = 1
        lab = np.zeros(m, np.uint8)
        if kind == 0:                       # several positives
            lab[rng.choice(m, size=int(rng.integers(2, 6)), replace=False)] = 1
        elif kind == 1:                     # no positive
            pass
        elif kind == 2:                     # only positives
            lab[:] = 1
        elif kind == 3:                     # fewer candidates than the largest k
            lab[int(rng.integers(0, m))] = 1
        elif kind == 4:                     # one sample, either class
            lab[0] = int(rng.random() < 0.5)
        else:
            lab[rng.random(m) < 0.5] = 1
        uids.append(np.full(m, u, np.int64)); labs.append(lab); lengths.append(m)
    uid, lab, sc = np.concatenate(uids), np.concatenate(labs), _codes(rng, lengths, 64)
    # interleave the users at random; each user's samples keep their order (they take its slots in order)
    slots = rng.permutation(uid.size)
    where = np.empty(uid.size, np.int64)
    for u in range(600):
        src = np.nonzero(uid == u)[0]
        where[src] = np.sort(slots[src])
    out_uid, out_lab, out_sc = np.empty_like(uid), np.empty_like(lab), np.empty_like(sc)
    out_uid[where], out_lab[where], out_sc[where] = uid, lab, sc
    return out_uid, out_lab, out_sc


def _sparse(rng):
    """5 000 users drawn from an id space of 200 000, 2..14 candidates each, in ascending id order."""
    ids = np.sort(rng.choice(200_000, size=5000, replace=False)).astype(np.int64)
    lengths = rng.integers(2, 15, ids.size)
    uid = np.repeat(ids, lengths)
    lab = np.zeros(uid.size, np.uint8)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    lab[starts + (rng.random(ids.size) * lengths).astype(np.int64)] = 1
    lab[rng.random(uid.size) < 0.05] = 1
    return uid, lab, _codes(rng, lengths, 32)


def _strided(arrays, stride):
    n = arrays[0].size
    assert np.gcd(stride, n) == 1
    src = (np.arange(n, dtype=np.int64) * stride) % n
    return tuple(x[src] for x in arrays)


def _groups(uid, scores, labels):
    """Per-user lists in first-appearance order (the grouping of trainer.py:311-320)."""
    order = {}
    for i, u in enumerate(uid.tolist()):
        order.setdefault(u, []).append(i)
    return [scores[v] for v in order.values()], [labels[v] for v in order.values()]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__.rsplit("usage: ", 1)[1])
    Trainer, RankingEvaluator = _reference(sys.argv[1])
    rng = np.random.default_rng(20261016)
    stride = 37_813                               # prime, coprime to 943 * 100
    # name: (samples (uid, labels, codes) or (base case, stride), code levels, ks)
    cases = {
        "loo_contiguous": (_loo(rng, 943, 100), 128, [1, 5, 10, 20]),
        "loo_shuffled": (("loo_contiguous", stride), 128, [1, 5, 10, 20]),
        "mixed": (_mixed(rng), 64, [1, 5, 10, 20]),
        "sparse_ids": (_sparse(rng), 32, [1, 5, 10, 20]),
        "large_ks": (_loo(rng, 100, 120), 128, [3, 50, 1000]),
    }
    out = {"cases": np.array(list(cases))}
    for name, (data, levels, ks) in cases.items():
        scale = 1.0 / levels
        if isinstance(data[0], str):
            base, st = data
            uid, lab, codes = _strided(cases[base][0], st)
            out.update({f"{name}/base": np.array(base), f"{name}/stride": np.array(st, np.int64)})
        else:
            uid, lab, codes = data
            out.update({f"{name}/user_ids": uid, f"{name}/labels": lab, f"{name}/score_codes": codes,
                        f"{name}/score_scale": np.array(scale)})
        sc = (codes.astype(np.float64) * scale).astype(np.float32)
        lf = lab.astype(np.float32)
        gs, gl = _groups(uid, sc, lf)
        assert all(np.unique(s).size == s.size for s in gs), f"{name}: tied scores within a user"
        me = types.SimpleNamespace(ranking_evaluator=RankingEvaluator(ks))
        ds = types.SimpleNamespace(features={"user_id": uid})
        trainer = Trainer._compute_ranking_metrics(me, ds, sc, lf)
        evaluator = RankingEvaluator(ks).evaluate(gs, gl)
        out.update({f"{name}/ks": np.array(ks, np.int32),
                    f"{name}/trainer": np.array(json.dumps({k: float(v) for k, v in trainer.items()})),
                    f"{name}/evaluator": np.array(json.dumps({k: float(v) for k, v in evaluator.items()}))})
        print(name, uid.size, trainer, flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ranking_reference.npz"), **out)


if __name__ == "__main__":
    main()
