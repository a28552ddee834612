"""The flash-attention builders of the runtime core -- ggml_flash_attn_ext, ggml_flash_attn_ext_set_prec
(src/ggml.c:6494-6549): the node each makes equals the reference library's in type, op, ne, nb,
op_params and sources.
"""
import ctypes
import os
import struct

import pytest

from conftest import REPO
from ggml_mi355x import ggml as G

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libggml_ref.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="make -C oracle ref")

F32, F16 = G.GGML_TYPE_F32, G.GGML_TYPE_F16
BUILDERS = ("ggml_flash_attn_ext", "ggml_flash_attn_ext_set_prec")


def _addr(t):
    return ctypes.cast(t, ctypes.c_void_p).value


def _describe(t, known):
    c = t.contents
    who = lambda p: known.get(p, "?") if p else None
    return dict(type=c.type, op=c.op, ne=tuple(c.ne), nb=tuple(c.nb), op_params=tuple(c.op_params), view_offs=c.view_offs,
                view_src=who(c.view_src), src=[who(c.src[i]) for i in range(10)], grad=bool(c.grad))


def _fa(D, N, nh, nh_kv, kv, mask, max_bias, ne3=1, ne3_kv=1, prec=None, mask_rows=None):
    def build(L, c):
        q = L.ggml_new_tensor_4d(c, F32, D, N, nh, ne3)
        k = L.ggml_new_tensor_4d(c, F16, D, kv, nh_kv, ne3_kv)
        v = L.ggml_new_tensor_4d(c, F16, D, kv, nh_kv, ne3_kv)
        ts = {"q": q, "k": k, "v": v}
        m = None
        if mask:
            rows = mask_rows or -(-N // G.GGML_KQ_MASK_PAD) * G.GGML_KQ_MASK_PAD
            m = L.ggml_new_tensor_2d(c, F16, kv, rows)
            ts["mask"] = m
        r = L.ggml_flash_attn_ext(c, q, k, v, m, 1.0 / D ** 0.5, max_bias)
        if prec is not None:
            L.ggml_flash_attn_ext_set_prec(r, prec)
        ts["r"] = r
        return ts
    return build


CASES = {
    "mask": _fa(128, 8, 32, 32, 96, True, 0.0),
    "no_mask": _fa(64, 1, 32, 32, 512, False, 0.0),
    "alibi": _fa(80, 4, 12, 12, 1024, True, 8.0),
    "gqa_4": _fa(128, 1, 32, 8, 4096, True, 0.0),
    "gqa_all": _fa(256, 33, 8, 1, 97, True, 0.0, mask_rows=96),
    "batch_bcast": _fa(96, 3, 8, 2, 64, True, 8.0, ne3=2, ne3_kv=1),
    "prec_f32": _fa(112, 2, 8, 4, 40, False, 0.0, prec=G.GGML_PREC_F32),
    "prec_default": _fa(128, 2, 8, 4, 40, True, 0.0, prec=G.GGML_PREC_DEFAULT),
}


def _nodes(L, build):
    with G.Context(L, L.ggml_tensor_overhead() * 8, no_alloc=True) as c:
        ts = build(L, c.ctx)
        known = {_addr(t): name for name, t in ts.items()}
        return {name: _describe(t, known) for name, t in ts.items()}


def _f32_bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def test_bindings_exist():
    rt = G.runtime()
    for name in BUILDERS:
        assert rt.has(name), name
    assert G.GGML_KQ_MASK_PAD == 32
    r = _nodes(rt, CASES["mask"])["r"]
    assert r["op"] == G.GGML_OP_FLASH_ATTN_EXT
    assert rt.ggml_op_name(r["op"]) == b"FLASH_ATTN_EXT"


def test_node_shape():
    d = _nodes(G.runtime(), CASES["gqa_4"])
    r = d["r"]
    # the permute(0, 2, 1, 3) of [D, N, nh]: [D, nh, N], contiguous f32
    assert r["type"] == F32 and r["ne"] == (128, 32, 1, 1) and r["nb"] == (4, 512, 16384, 16384)
    assert r["src"][:5] == ["q", "k", "v", "mask", None]
    assert r["op_params"][0] == _f32_bits(1.0 / 128 ** 0.5) and r["op_params"][1] == 0 and r["op_params"][2] == 0
    assert not r["grad"] and r["view_src"] is None
    d = _nodes(G.runtime(), CASES["no_mask"])
    assert d["r"]["src"][:4] == ["q", "k", "v", None]
    d = _nodes(G.runtime(), CASES["alibi"])
    assert d["r"]["op_params"][1] == _f32_bits(8.0)
    d = _nodes(G.runtime(), CASES["prec_f32"])
    assert d["r"]["op_params"][2] == G.GGML_PREC_F32
    d = _nodes(G.runtime(), CASES["batch_bcast"])
    assert d["r"]["ne"] == (96, 8, 3, 2)


@needs_ref
@pytest.mark.parametrize("case", list(CASES))
def test_node_equals_reference(case):
    ref = G.Lib([REF_LIB], isolated=True)
    assert ref.has("ggml_flash_attn_ext")
    ours, theirs = _nodes(G.runtime(), CASES[case]), _nodes(ref, CASES[case])
    assert ours == theirs
    assert ours["r"]["op"] == G.GGML_OP_FLASH_ATTN_EXT
