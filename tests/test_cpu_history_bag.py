"""CPU: the declarations behind history bags that are formed at record assembly (DESIGN.md §7b "History bags at record
assembly"): ``dfm_history_source`` and ``dfm_assemble_plan_bind_history`` in the header against their ctypes binding,
the ABI version that must not move, and the argument checks of ``HistoryBag`` / ``DeviceColumns.from_device`` that are
raised before any device work.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from deepfm_amd import _lib
from deepfm_amd.data import interactions as I
from tests.test_cpu_history import _bare_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "deepfm_hip.h")).read()
CTYPES = {"const int64_t*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64,
          "int32_t": ctypes.c_int32}
SIZES = {ctypes.c_void_p: 8, ctypes.c_int64: 8, ctypes.c_int32: 4}


def _struct_members(name):
    """(type, member) pairs of ``typedef struct name { ... } name;`` as the header declares them."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [tuple(m.strip().rsplit(" ", 1)) for m in body.split(";") if m.strip()]


def test_the_header_declares_the_struct_and_the_entry_point_and_the_binding_matches():
    members = _struct_members("dfm_history_source")
    assert [m for _, m in members] == ["d_user_rows", "d_item_rows", "d_timestamps", "d_item_ids", "d_start",
                                       "d_pos_of", "d_rank", "d_events", "d_sorted_ts", "d_event_count", "n",
                                       "n_users", "n_items", "mode"]
    fields = _lib.HistorySource._fields_
    assert [name for name, _ in fields] == [m for _, m in members]
    assert [ctype for _, ctype in fields] == [CTYPES[t] for t, _ in members]
    # the C layout: every member at its natural alignment, the size rounded up to the widest member's
    offset = 0
    for name, ctype in fields:
        offset = (offset + SIZES[ctype] - 1) // SIZES[ctype] * SIZES[ctype]
        assert getattr(_lib.HistorySource, name).offset == offset, name
        offset += SIZES[ctype]
    assert ctypes.sizeof(_lib.HistorySource) == (offset + 7) // 8 * 8 == 112
    assert ("int dfm_assemble_plan_bind_history(dfm_assemble_plan* plan, int column, const dfm_history_source* source);"
            in HEADER)
    restype, argtypes = _lib.SIGNATURES["dfm_assemble_plan_bind_history"]
    assert restype is _lib._I and argtypes == [_lib._P, _lib._I, ctypes.POINTER(_lib.HistorySource)]
    lib = _lib.load()
    assert lib.dfm_assemble_plan_bind_history.argtypes == argtypes


def test_the_abi_version_and_the_existing_layouts_stay():
    assert _lib.ABI_VERSION == 11 and _lib.load().dfm_abi_version() == 11
    assert "#define DFM_ABI_VERSION 11 " in HEADER
    members = [m for _, m in _struct_members("dfm_assemble_column")]
    assert members == ["kind", "role", "length", "num_edges", "record_offset", "pos", "item", "ctx", "edges",
                       "bucket_ids"] == [name for name, _ in _lib.AssembleColumn._fields_]
    assert ctypes.sizeof(_lib.AssembleColumn) == 64
    assert "int dfm_record_assemble(const dfm_assemble_plan* plan, const int64_t* d_order, int64_t first," in HEADER


def test_the_entry_point_refuses_null_arguments_without_a_device():
    lib = _lib.load()
    src = _lib.HistorySource()
    assert lib.dfm_assemble_plan_bind_history(None, 0, src) == 1
    assert "null argument" in lib.dfm_last_error().decode()
    assert lib.dfm_assemble_plan_bind_history(0x1000, 0, None) == 1
    assert "null argument" in lib.dfm_last_error().decode()


def test_history_bag_refuses_bad_arguments_by_name_before_the_device():
    from deepfm_amd.data import HistoryBag
    ix = _bare_index()
    good = torch.zeros(3, dtype=torch.int64)
    for ties in ("first", "", None, "newest"):
        with pytest.raises(ValueError, match=r"ties = .*: expected one of \('position', 'exclude', 'latest'\)"):
            HistoryBag(ix, good, 5, ties=ties)
    for bad in (0, -1, _lib.HISTORY_MAX_LENGTH + 1, 2.0, True, None):
        with pytest.raises(ValueError, match=r"length = .* outside \[1, 4096\]"):
            HistoryBag(ix, good, bad)
    with pytest.raises(TypeError, match="queries: expected torch.int64"):
        HistoryBag(ix, good.to(torch.int32), 5)
    with pytest.raises(ValueError, match="queries: expected one axis"):
        HistoryBag(ix, good.reshape(3, 1), 5)
    with pytest.raises(TypeError, match="queries: expected a torch tensor"):
        HistoryBag(ix, np.zeros(3, np.int64), 5)
    with pytest.raises(ValueError, match="queries is on cpu, the log on cuda"):
        HistoryBag(ix, good, 5, ties="latest")
    with pytest.raises(ValueError, match="fewer than 2\\^31"):
        HistoryBag(ix, torch.zeros(1, dtype=torch.int64).expand(2**31), 1)
    # 4.6 GB of bags: the size is no reason to refuse (the next check speaks: the tensor is on the host)
    m = I.HISTORY_MAX_BYTES // (8 * 4096) + 1
    with pytest.raises(ValueError, match="queries is on cpu"):
        HistoryBag(ix, torch.zeros(1, dtype=torch.int64).expand(m), 4096)
    assert I.HISTORY_BAG_TIES == ("position", "exclude", "latest") and I.HISTORY_TIES == ("position", "exclude")


def _bare_bag(n, length):
    from deepfm_amd.data import HistoryBag
    bag = HistoryBag.__new__(HistoryBag)
    bag.queries, bag.length, bag.ties = torch.zeros(n, dtype=torch.int64), length, "position"
    return bag


def test_from_device_takes_a_history_bag_and_refuses_one_of_another_shape():
    from deepfm_amd.data import DeviceColumns, history_field
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    n, L = 7, 5
    schema = DatasetSchema(fields={"user_id": FieldSchema("user_id", FeatureType.SPARSE, 10, 8, "user"),
                                   "hist": history_field("hist", L, 40, 8)})
    ids, dense = torch.zeros(1, n, dtype=torch.int64), torch.zeros(0, n)
    labels = torch.zeros(n)
    bag = _bare_bag(n, L)
    cols = DeviceColumns.from_device(schema, ids, dense, labels, bags=[bag])
    assert len(bag) == n and cols.bags == [bag] and cols.field_columns()["hist"] is bag
    assert cols.field_columns()["user_id"].data_ptr() == ids.data_ptr()
    with pytest.raises(ValueError, match=f"bag of 'hist': expected a HistoryBag of {n} queries and length {L} on cpu, "
                                         f"got {n + 1} queries and length {L}"):
        DeviceColumns.from_device(schema, ids, dense, labels, bags=[_bare_bag(n + 1, L)])
    with pytest.raises(ValueError, match=f"bag of 'hist': expected a HistoryBag of {n} queries and length {L} on cpu, "
                                         f"got {n} queries and length {L + 1}"):
        DeviceColumns.from_device(schema, ids, dense, labels, bags=[_bare_bag(n, L + 1)])
    with pytest.raises(ValueError, match="bag of 'hist': expected a contiguous torch.int64 tensor"):      # as before
        DeviceColumns.from_device(schema, ids, dense, labels, bags=[torch.zeros(n, L + 1, dtype=torch.int64)])
