"""Every compiled instance of search_kernel (csrc/bang_search.hip: twelve pivot layouts x code rows dword-aligned or not), in every form of the
BANG_Base walk and in the BANG_Inmemory build, on the layout list of tests/instance_inputs.py -- against oracle.Oracle.search (the Inmemory build:
tests/inmemory_reference.py), bit for bit: ids, distance bits and the four per-query counters.  Every engine reports the code stride its entry
asked for: that is what proves which ALIGNED variant ran.  tests/test_instance_inputs.py asserts on the CPU that the list reaches the instances.

What the engine gives no way to observe: bang_get_stats reports neither the pivot table bang_alloc took (pq_nhi) nor the SPEC variant.  That the
218 / 219 entries with pq_ragged = 1 run the NHI = 58 / 22 instances rests on tests/test_instance_inputs.py restating bang_alloc's rule
(w_rag > w_pad, from bang_search_supported); if bang_alloc chose differently while that restated rule still held, both kinds of entry would run
the padded table and stay green here."""
import numpy as np
import pytest

import base_forms as F
import edge_inputs as E
import instance_inputs as I
from inmemory_reference import Reference

pytestmark = pytest.mark.gpu

NO_UNALIGNED_128 = r"semantics = 1 \(inmemory\): no kernel instance for 128-chunk code rows that are not dword-aligned"
_REF = {}


def _oracle(e, q, k, L):
    """Oracle.search(..., with_stats=True), once per (shape, queries, k, L): entries that differ in the options share it."""
    from oracle import oracle as O
    key = (I.shape_of(e), q.shape[0], k, L)
    if key not in _REF:
        _REF[key] = O.Oracle(I.entry_index(e)[0]).search(q, k, L, with_stats=True)
    return _REF[key]


def _inmemory(e, q, L):
    """The Inmemory reference at k = L; a smaller k is a prefix of it (edge_inputs.first_k)."""
    key = (I.shape_of(e), "inmemory", L)
    if key not in _REF:
        _REF[key] = Reference(I.entry_index(e)[0]).search(q, L, L, "inmemory")
    return _REF[key]


def _cases(groups, entries=I.ENTRIES):
    return [pytest.param(e, g, id=f"{I.entry_id(e)}-{g}") for e in entries for g in groups]


# ---------------------------------------------------------------------------------------------------------------------
# the forms of the BANG_Base walk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,group", _cases(F.GROUPS))
def test_instance_in_every_form(entry, group, monkeypatch):
    ix, q = I.entry_index(entry)
    for form in F.forms_of(group, ix.dtype, ix.D, ix.R, ix.N):
        with F.open_engine(ix, form, monkeypatch, **I.options_of(entry)) as e:
            for k, L in I.runs_of(entry):
                F.assert_same(F.run(e, form, q, k, L), _oracle(entry, q, k, L), form)
                F.assert_form(e, form, ix, q.shape[0], L, code_stride=I.stride_of(entry))
                e.free()
            e.unload()


@pytest.mark.parametrize("entry", [e for e in I.ENTRIES if e.key in (218, 219)], ids=I.entry_id)
@pytest.mark.parametrize("spec_rows", ("1", "2"))
def test_speculative_row_request_on_and_off(entry, spec_rows, monkeypatch):
    """BANG_SPEC_ROWS: the code rows of all ids of an adjacency row requested with their filter probes (1: the SPEC instances, which exist for 18
    and 19 code dwords only) or behind the filter (2).  Same results -- and that is all this can show: no statistic names the variant that ran.
    With the few queries of these entries the launch policy (spec_auto, bang_k_search) is on already, so "1" repeats what the other tests of
    this file run on these entries; "2" is the leg that adds an instance, SPEC = false."""
    ix, q = I.entry_index(entry)
    monkeypatch.setenv("BANG_SPEC_ROWS", spec_rows)
    for form in ("self_fused", "pull_host"):
        with F.open_engine(ix, form, monkeypatch, **I.options_of(entry)) as e:
            for k, L in I.runs_of(entry)[1:]:
                F.assert_same(F.run(e, form, q, k, L), _oracle(entry, q, k, L), form)
                F.assert_form(e, form, ix, q.shape[0], L, code_stride=I.stride_of(entry))
                e.free()
            e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# launch shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,form", _cases(("self_fused", "pull_host"), [e for e in I.ENTRIES if e.key in I.LAUNCH_SHAPE_KEYS]))
def test_launch_shape_does_not_change_results(entry, form, monkeypatch):
    ix, q = I.entry_index(entry)
    k, L = 10, 37
    ref = _oracle(entry, q, k, L)
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")                    # one wave runs every query in turn
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    with F.open_engine(ix, form, monkeypatch, **I.options_of(entry)) as e:
        F.assert_same(F.run(e, form, q, k, L), ref, form)
        F.assert_form(e, form, ix, q.shape[0], L, code_stride=I.stride_of(entry))
        e.free()
        e.unload()
    monkeypatch.delenv("BANG_SEARCH_MAX_WGS")
    monkeypatch.delenv("BANG_SEARCH_MAX_WAVES")
    with F.open_engine(ix, form, monkeypatch, **I.options_of(entry)) as e:        # batches of 1, 7 and all on one allocation
        e.set_searchparams(k, L)
        e.alloc(q.shape[0])
        for nb in (1, 7, q.shape[0]):
            e.init(nb)
            ids, d = e.query(q[:nb])
            F.assert_same((ids, d, e.query_counters(nb)), (ref[0][:nb], np.ascontiguousarray(ref[1][:, :nb]), ref[2][:nb]), form)
            F.assert_form(e, form, ix, nb, L, code_stride=I.stride_of(entry))
        e.free()
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# the Inmemory build of the same instances
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", I.ENTRIES, ids=I.entry_id)
def test_inmemory_build(entry):
    """semantics = 1 repeats the whole set of instances, except 128-chunk rows that are not dword-aligned (bang_search_inmem_has_instance): that
    entry is refused, with the message that names the way out."""
    import bang_amd
    ix, q = I.entry_index(entry)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, semantics=bang_amd.SEMANTICS_INMEMORY, **I.options_of(entry)) as e:
        e.load_index(ix)
        if entry.key == 132 and not I.aligned(entry):
            e.set_searchparams(10, 37)
            with pytest.raises(bang_amd.BangError, match=NO_UNALIGNED_128):
                e.alloc(q.shape[0])
            return
        for k, L in I.runs_of(entry):
            e.set_searchparams(k, L)
            e.alloc(q.shape[0])
            e.init(q.shape[0])
            ids, d = e.query(q)
            F.assert_same((ids, d, e.query_counters(q.shape[0])), E.first_k(_inmemory(entry, q, L), k))
            s = e.stats()
            assert s["search_kernel"] == 1 and s["front_launches"] == 1 and s["code_stride"] == I.stride_of(entry), s
            e.free()
        e.unload()
