"""CPU checks of the entry points of branch-and-bound node and child assembly, the parent store and the batched read-back
(lpx_tableau_build_node / _nodes / _child / _child_from_store / _children_from_store, lpx_store_*, lpx_multi_solution): exported
and declared, mirrored in C# and Python, and argument errors answered before any device is looked for."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_tableau_build_node", "lpx_tableau_build_nodes", "lpx_tableau_build_child", "lpx_tableau_build_child_from_store",
           "lpx_tableau_build_children_from_store", "lpx_store_create", "lpx_store_destroy", "lpx_store_save", "lpx_store_release",
           "lpx_store_save_multi", "lpx_multi_solution", "lpx_tableau_shape", "lpx_tableau_set_shape")


def test_symbols_exported_declared_and_mirrored(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s          # a ctypes signature in _lib.py
        assert re.search(r"\b%s\(" % s, hdr), s
        assert (" %s(" % s) in native, s
    assert L.lpx_abi_version() == 1


def test_argument_errors_come_first(lpx):
    """Checked before any device is looked for and before any handle is read: the same answers with and without a GPU.  The
    handles passed where a later argument is the wrong one are never dereferenced: zeroed memory stands in for them."""
    L = lpx._lib.lib()
    EINVAL, ip, dp, vp = lpx._lib.EINVAL, lpx._lib.ip, lpx._lib.dp, C.c_void_p
    blank = C.create_string_buffer(4096)
    h = C.cast(blank, vp)
    hs = (vp * 2)(h, h)
    var = np.zeros(2, dtype=np.int32); d = np.zeros(2); off = np.array([0, 1, 2], dtype=np.int32)
    vpt, dpt, opt = var.ctypes.data_as(ip), d.ctypes.data_as(dp), off.ctypes.data_as(ip)
    slots = (C.c_int * 2)()

    def refused(rc, what):
        assert rc == EINVAL and what in lpx._lib.last_error(), (rc, lpx._lib.last_error())

    # cold nodes
    refused(L.lpx_tableau_build_node(None, h, 0, None, None, None, None), "lpx_tableau_build_node: bad argument")
    refused(L.lpx_tableau_build_node(h, None, 0, None, None, None, None), "lpx_tableau_build_node: bad argument")
    refused(L.lpx_tableau_build_node(h, h, -1, vpt, dpt, dpt, dpt), "lpx_tableau_build_node: bad argument")
    for args in ((None, dpt, dpt, dpt), (vpt, None, dpt, dpt), (vpt, dpt, None, dpt), (vpt, dpt, dpt, None)):
        refused(L.lpx_tableau_build_node(h, h, 2, *args), "lpx_tableau_build_node: bad argument")
    refused(L.lpx_tableau_build_nodes(None, h, 2, opt, vpt, dpt, dpt, dpt), "lpx_tableau_build_nodes: bad argument")
    refused(L.lpx_tableau_build_nodes(hs, None, 2, opt, vpt, dpt, dpt, dpt), "lpx_tableau_build_nodes: bad argument")
    refused(L.lpx_tableau_build_nodes(hs, h, -1, opt, vpt, dpt, dpt, dpt), "lpx_tableau_build_nodes: bad argument")
    refused(L.lpx_tableau_build_nodes(hs, h, 2, None, vpt, dpt, dpt, dpt), "lpx_tableau_build_nodes: bad argument")
    bad_off = np.array([1, 1, 2], dtype=np.int32)
    refused(L.lpx_tableau_build_nodes(hs, h, 2, bad_off.ctypes.data_as(ip), vpt, dpt, dpt, dpt), "lpx_tableau_build_nodes: bad cut arrays")
    neg_off = np.array([0, 1, -1], dtype=np.int32)
    refused(L.lpx_tableau_build_nodes(hs, h, 2, neg_off.ctypes.data_as(ip), vpt, dpt, dpt, dpt), "lpx_tableau_build_nodes: bad cut arrays")
    for args in ((None, dpt, dpt, dpt), (vpt, None, dpt, dpt), (vpt, dpt, None, dpt), (vpt, dpt, dpt, None)):
        refused(L.lpx_tableau_build_nodes(hs, h, 2, opt, *args), "lpx_tableau_build_nodes: bad cut arrays")
    assert L.lpx_tableau_build_nodes(hs, h, 0, opt, None, None, None, None) == 0            # an empty group is no error
    # warm children
    refused(L.lpx_tableau_build_child(None, h, 0, 0, 0, 1.0), "lpx_tableau_build_child: bad argument")
    refused(L.lpx_tableau_build_child(h, None, 0, 0, 0, 1.0), "lpx_tableau_build_child: bad argument")
    refused(L.lpx_tableau_build_child(h, h, 0, 0, 0, 1.0), "lpx_tableau_build_child: bad argument")       # the parent itself
    refused(L.lpx_tableau_build_child_from_store(None, h, 0, 0, 0, 0, 1.0), "lpx_tableau_build_child_from_store: bad argument")
    refused(L.lpx_tableau_build_child_from_store(h, None, 0, 0, 0, 0, 1.0), "lpx_tableau_build_child_from_store: bad argument")
    ok = (hs, hs, slots, 2, vpt, vpt, vpt, dpt)
    for k in (0, 1, 2, 4, 5, 6, 7):
        args = list(ok); args[k] = None
        refused(L.lpx_tableau_build_children_from_store(*args), "lpx_tableau_build_children_from_store: bad argument")
    args = list(ok); args[3] = -1
    refused(L.lpx_tableau_build_children_from_store(*args), "lpx_tableau_build_children_from_store: bad argument")
    assert L.lpx_tableau_build_children_from_store(hs, hs, slots, 0, None, None, None, None) == 0
    # the store
    out = vp()
    for Rcap, Ccap in ((1, 8), (0, 8), (-3, 8), (4, 1)):
        refused(L.lpx_store_create(Rcap, Ccap, C.byref(out)), "lpx_store_create: bad shape")
    refused(L.lpx_store_create(4, 8, None), "lpx_store_create: bad shape")
    assert not out.value
    one = C.c_int(-7)
    refused(L.lpx_store_save(None, h, C.byref(one)), "lpx_store_save: null argument")
    refused(L.lpx_store_save(h, None, C.byref(one)), "lpx_store_save: null argument")
    refused(L.lpx_store_save(h, h, None), "lpx_store_save: null argument")
    assert one.value == -7
    assert L.lpx_store_release(None, 0) == EINVAL
    for args in ((None, hs, 2, slots), (hs, None, 2, slots), (hs, hs, 2, None), (hs, hs, -1, slots)):
        refused(L.lpx_store_save_multi(*args), "lpx_store_save_multi: bad argument")
    nulls = (vp * 2)()
    refused(L.lpx_store_save_multi(nulls, hs, 2, slots), "lpx_store_save_multi: null argument")
    refused(L.lpx_store_save_multi(hs, nulls, 2, slots), "lpx_store_save_multi: null argument")
    assert L.lpx_store_save_multi(hs, hs, 0, slots) == 0
    L.lpx_store_destroy(None)
    # the read-back
    x = np.zeros(4); z = np.zeros(2)
    refused(L.lpx_multi_solution(None, 2, 2, x.ctypes.data_as(dp), z.ctypes.data_as(dp), None, 0), "lpx_multi_solution: bad argument")
    refused(L.lpx_multi_solution(hs, -1, 2, x.ctypes.data_as(dp), z.ctypes.data_as(dp), None, 0), "lpx_multi_solution: bad argument")
    refused(L.lpx_multi_solution(hs, 2, -1, x.ctypes.data_as(dp), z.ctypes.data_as(dp), None, 0), "lpx_multi_solution: bad argument")
    refused(L.lpx_multi_solution(nulls, 2, 2, x.ctypes.data_as(dp), z.ctypes.data_as(dp), None, 0), "lpx_multi_solution: null or empty tableau")
    assert L.lpx_multi_solution(hs, 0, 2, None, None, None, 0) == 0
    assert L.lpx_tableau_shape(None, None, None, None) == EINVAL
    refused(L.lpx_tableau_set_shape(None, 2, 4), "lpx_tableau_set_shape: shape outside the handle's capacity")
