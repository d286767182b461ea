"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/snerf_hip.h declares, and its host-only entry points behave (no GPU work here)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(snerf_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from snerf_amd import _lib
    L = _lib.lib()
    declared = _declared_symbols()
    assert len(declared) >= 9
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/snerf_hip.h but not exported"
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared


_SCALARS = {"int": ("int", 4, True), "unsigned": ("int", 4, False), "long long": ("int", 8, True),
            "unsigned long long": ("int", 8, False), "size_t": ("int", 8, False), "float": ("float", 4, True),
            "double": ("float", 8, True)}


def _c_type(text):
    """a C parameter or return type -> ("pointer", pointee) or (class, bytes, signed)"""
    words = text.replace("*", " * ").split()
    base = " ".join(w for w in words if w not in ("const", "*"))
    return ("pointer", base) if "*" in words else _SCALARS[base]


def _header_prototypes():
    """include/snerf_hip.h without comments, preprocessor lines and struct bodies -> {symbol: (return type, [(type, name)])}"""
    src = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", src, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(snerf_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        params = [] if params.strip() == "void" else [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        protos[name] = (_c_type(ret), [(_c_type(t), n) for t, n in params])
    return protos


def _table_type(t):
    """a ctypes type of the table, in _c_type's terms"""
    from snerf_amd import _lib
    if t is C.c_char_p:
        return ("pointer", "char")
    if issubclass(t, C.c_void_p):
        return ("pointer", None)                       # void*: stands for a pointer to anything (device memory, host tables)
    if issubclass(t, C._Pointer):
        inner = t._type_
        if issubclass(inner, C.Structure):
            assert getattr(_lib, inner.__name__) is inner
            return ("pointer", inner.__name__)
        return ("pointer", {v: k for k, v in _SCALARS.items()}[_table_type(inner)])
    if t in (C.c_float, C.c_double):
        return ("float", C.sizeof(t), True)
    return ("int", C.sizeof(t), t(-1).value < 0)


def test_binding_table_matches_header_prototypes():
    """Every prototype of the header against its row of _lib.SIGNATURES: the return type, the parameter count and, per parameter,
    class, width and signedness; a pointer to a struct against POINTER() of the mirror with that name (or void*); the stream
    marker exactly where the header's parameter is called `stream`.  No symbol is left out: the parser must give a prototype
    for every name _declared_symbols() finds; the rows stand in the header's order."""
    from snerf_amd import _lib
    protos = _header_prototypes()
    assert sorted(protos) == _declared_symbols() == sorted(_lib.SIGNATURES) and len(protos) >= 53
    assert list(_lib.SIGNATURES) == list(protos)                    # the header's declaration order, for the whole table
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert _table_type(restype) == ret, (name, "return type", restype, ret)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (t, (want, pname)) in enumerate(zip(argtypes, params)):
            got = _table_type(t)
            assert got == want or (want[0] == "pointer" and got == ("pointer", None)), (name, k, pname, t, want)
            assert (t is _lib.c_stream) == (pname == "stream"), (name, k, pname, t)
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():       # lib() applied the table
        assert getattr(L, name).restype is restype and tuple(getattr(L, name).argtypes) == tuple(argtypes), name
        assert name in _lib._PLANS                                  # _lib.call works by name


def test_call_argument_handling_without_a_launch():
    """_lib.call refuses what must not reach the library before anything is launched, and direct callers of lib() can still
    hand a stream slot what a void* takes."""
    import torch
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    rays, steps, z = torch.zeros(5, 8), torch.zeros(3), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match=r"must live on the GPU \(the HIP path has no CPU fallback\)"):
        _lib.call("snerf_sample_z", rays, steps, None, z, 5, 3)
    with pytest.raises(TypeError, match="snerf_sample_z takes 6 arguments"):
        _lib.call("snerf_sample_z", None, None, None, None, 5)
    with pytest.raises(TypeError, match="snerf_sample_z takes 6 arguments"):
        _lib.call("snerf_sample_z", None, None, None, None, 5, 3, None)        # the stream is not the caller's to pass
    with pytest.raises(TypeError, match="device"):
        _lib.call("snerf_sample_z", None, None, None, None, 5, 3)              # no tensor, no device=: no stream to take
    with pytest.raises(TypeError):
        _lib.call_size("snerf_workspace_bytes")
    d = ModelSpec().desc(64, 8)
    assert _lib.call_size("snerf_workspace_bytes", d) == _lib.lib().snerf_workspace_bytes(C.byref(d)) > 0
    for v in (None, 0, C.c_void_p(16), _lib.c_stream(16)):
        _lib.c_stream.from_param(v)


def test_struct_sizes_match_header():
    """ctypes mirrors must match the C layout (64-bit pointers, 4-byte ints)."""
    from snerf_amd import _lib
    assert C.sizeof(_lib.SnerfDesc) == 16 * 4
    assert C.sizeof(_lib.SnerfParams) == 8 * (2 * 16 + 12 + 8 + 12)
    assert C.sizeof(_lib.SnerfInputs) == 8 * 9
    assert C.sizeof(_lib.SnerfOutputs) == 8 * 13
    assert C.sizeof(_lib.SnerfOutGrads) == 8 * 11


def test_host_only_sizes_and_errors():
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    spec = ModelSpec()
    d = spec.desc(4096, 64, _lib.FLAG_TRAIN)
    n = L.snerf_packed_floats(C.byref(d))
    # 2,826,766 parameters + padding of the packed layout, then one two-plane WF16 pack per weight operand (every
    # matrix and its transpose for dX: 4 bytes per element each)
    assert 3 * 2_800_000 < n < 15_000_000
    d1 = spec.desc(4096, 64, _lib.FLAG_TRAIN | _lib.FLAG_F16X1)
    n1 = L.snerf_packed_floats(C.byref(d1))
    assert 2 * 2_800_000 < n1 < n                                          # one-plane packs: half the bytes behind the fp32 region
    assert L.snerf_grad_floats(C.byref(d1)) == L.snerf_grad_floats(C.byref(d))
    train = L.snerf_workspace_bytes(C.byref(d))
    d.flags = 0
    infer = L.snerf_workspace_bytes(C.byref(d))
    assert 0 < infer < train < 20 * 2**30
    bad = spec.desc(0, 64)
    assert L.snerf_workspace_bytes(C.byref(bad)) == 0
    assert b"n_rays" in L.snerf_last_error()
    bad = ModelSpec(fc_units=520).desc(16, 8)
    with pytest.raises(RuntimeError, match=r"snerf_packed_floats failed \(code 1\): .*fc_units"):      # a returned 0, through the binding
        _lib.call_size("snerf_packed_floats", bad)
    assert b"fc_units" in L.snerf_last_error()
    # the two arithmetic flags exclude each other (flags = 0 is the default arithmetic, f16x2)
    both = ModelSpec().desc(16, 8, _lib.FLAG_F16X2 | _lib.FLAG_F16X1)
    assert L.snerf_workspace_bytes(C.byref(both)) == 0 and b"arithmetic flag" in L.snerf_last_error()
    one = ModelSpec(fc_units=64, feat_last=32).desc(64, 8, _lib.FLAG_TRAIN | _lib.FLAG_F16X1)
    two = ModelSpec(fc_units=64, feat_last=32).desc(64, 8, _lib.FLAG_TRAIN)
    assert 0 < L.snerf_workspace_bytes(C.byref(one)) < L.snerf_workspace_bytes(C.byref(two))   # 2 bytes per stored activation element
    odd = ModelSpec(fc_units=96, feat_last=48).desc(16, 8, _lib.FLAG_F16X1)                       # one plane: LDS stages of 64 columns
    assert L.snerf_workspace_bytes(C.byref(odd)) == 0 and b"fc_units % 64" in L.snerf_last_error()
    assert L.snerf_workspace_bytes(C.byref(ModelSpec(fc_units=96, feat_last=48).desc(16, 8))) > 0
    # the default arithmetic is the same object for a C caller (flags = 0) and for Python's ModelSpec()
    assert L.snerf_workspace_bytes(C.byref(ModelSpec().desc(64, 8))) == L.snerf_workspace_bytes(C.byref(ModelSpec().desc(64, 8, _lib.FLAG_F16X2)))
    assert L.snerf_version() == 6


def test_plan_builder_over_model_variants_and_null_arguments():
    """The host code behind the C-ABI (plan / table builders, argument checks) over every model variant, pass kind and
    arithmetic; null and misaligned arguments of the hot calls come back as error codes with a message, never as a crash.
    `make -C snerf_amd/csrc asan-test` runs this file against the ASAN + UBSAN host build of the library."""
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    seen = set()
    for kw in ({}, {"siren": False}, {"model": "satnerf"} if "model" in ModelSpec.__dataclass_fields__ else {},
               {"use_separate_beta_for_s": True}, {"use_tj_for_s": True}, {"use_tj_instead_of_beta": True}, {"fc_units": 64}, {"fc_units": 128, "fc_layers": 4, "fc_skips": (2,)}):
        try:
            spec = ModelSpec(**kw)
        except TypeError:
            continue
        for flags in (0, _lib.FLAG_TRAIN, _lib.FLAG_SC_PASS, _lib.FLAG_TRAIN | _lib.FLAG_SC_PASS, _lib.FLAG_TRAIN | _lib.FLAG_F16X1, _lib.FLAG_F16X1, _lib.FLAG_F16X1 | _lib.FLAG_TRAIN | _lib.FLAG_SC_PASS):
            for N, S in ((1, 1), (77, 7), (4096, 64), (2048, 130)):
                d = spec.desc(N, S, flags)
                n, g, w = L.snerf_packed_floats(C.byref(d)), L.snerf_grad_floats(C.byref(d)), L.snerf_workspace_bytes(C.byref(d))
                assert n > 0 and w > 0 and 0 < g <= n, (kw, flags, N, S, L.snerf_last_error())
                seen.add((n, g))
    assert len(seen) >= 4
    d = ModelSpec().desc(64, 8, _lib.FLAG_TRAIN)
    # hot calls with null / misaligned arguments: an error code and a message (no device work is reached)
    assert L.snerf_pack_params(C.byref(d), None, None, None) != 0 and L.snerf_last_error()
    assert L.snerf_forward(C.byref(d), None, None, None, None, 0, None) != 0
    assert L.snerf_backward(C.byref(d), None, None, None, None, None, None, None, 0, None) != 0
    assert L.snerf_unpack_grads(C.byref(d), None, None, 0, None) != 0
    assert L.snerf_grad_floats(None) == 0 and L.snerf_workspace_bytes(None) == 0
    bad = ModelSpec().desc(-5, 64)
    assert L.snerf_grad_floats(C.byref(bad)) == 0 and L.snerf_workspace_bytes(C.byref(bad)) == 0


def test_plan_sizes_are_frozen():
    """The layout the plan gives is part of what a refactor of the plan / pass host code must keep: the packed parameter buffer, the
    gradient buffer and the workspace of every recorded descriptor have the sizes of tests/golden/plan_sizes.json (recorded by
    tools/gen_golden_plan.py from a build of the commit named in the file), and every descriptor refused there is refused with
    the same message.  The sweep: the variants x flag sets x (N, S) of the test above, the five BASELINE.json shapes, 1 / 3 / 16 layers, a
    skip at the last layer, 0 / 9 / 16 classes, a width with no folded narrow projections, a separate t_s, both arithmetic modes."""
    import json
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_sizes.json")))
    assert doc["fields"] == [f for f, _ in _lib.SnerfDesc._fields_]
    cases = doc["cases"]
    assert len(cases) == 310 and sum(c["error"] is not None for c in cases) == 12
    assert {c["group"] for c in cases} == {"variants", "baseline", "shapes"}
    assert {(c["desc"][0], c["desc"][1]) for c in cases if c["group"] == "baseline"} == {(512, 32), (4096, 64), (8192, 96), (16384, 128), (32768, 128)}
    for c in cases:
        d = _lib.SnerfDesc(*c["desc"])
        spec = {k: tuple(v) if isinstance(v, list) else v for k, v in c["spec"].items()}
        again = ModelSpec(**spec).desc(d.n_rays, d.n_samples, d.flags)
        assert bytes(again) == bytes(d), c                               # the recorded descriptor is the one the spec gives today
        got = [L.snerf_packed_floats(C.byref(d)), L.snerf_grad_floats(C.byref(d)), L.snerf_workspace_bytes(C.byref(d))]
        assert got == c["sizes"], (c["spec"], c["desc"], got, c["sizes"])
        if c["error"] is not None:
            assert got == [0, 0, 0] and L.snerf_last_error().decode() == c["error"], (c["desc"], L.snerf_last_error())


def test_one_plane_mode_refuses_raw_xyz():
    """SNERF_FLAG_F16X1 with n_freq = 0 (SatNeRF's raw xyz) is refused by name: one fp16 plane rounds the coordinates entering the
    w0 = 30 first layer to 11 bits (sigma off by 5e-3 against the fp64 oracle).  The default arithmetic, and the one-plane mode with any
    positional encoding, keep their plans."""
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    raw = ModelSpec(n_freq=0, n_classes=0)
    for flags in (_lib.FLAG_F16X1, _lib.FLAG_F16X1 | _lib.FLAG_TRAIN, _lib.FLAG_F16X1 | _lib.FLAG_SC_PASS):
        d = raw.desc(512, 32, flags)
        assert L.snerf_packed_floats(C.byref(d)) == 0 and L.snerf_workspace_bytes(C.byref(d)) == 0
        assert b"raw xyz" in L.snerf_last_error(), L.snerf_last_error()
    for spec, flags in ((raw, 0), (raw, _lib.FLAG_TRAIN), (ModelSpec(n_freq=1), _lib.FLAG_F16X1), (ModelSpec(), _lib.FLAG_F16X1 | _lib.FLAG_TRAIN)):
        d = spec.desc(512, 32, flags)
        assert L.snerf_packed_floats(C.byref(d)) > 0 and L.snerf_workspace_bytes(C.byref(d)) > 0, (flags, L.snerf_last_error())


@pytest.mark.parametrize("kw,flags,msg", [
    ({"n_classes": 17}, 0, b"n_classes out of range"),                                     # MAX_CLASSES = 16
    ({"t_dim": 14}, 0, b"3 + t_dim"),                                                      # 3 + 14 > 16 columns of the extras block
    ({"t_dim": 7, "use_separate_tj_for_semantic": True, "use_tj_for_s": True}, 0, b"3 + t_dim"),   # 3 + 2 x 7 > 16
    ({"feat_last": 520}, 0, b"feat_last must be"),                                         # > 64 x MAX_SKY_UNITS
    ({"feat_last": 24}, 0, b"feat_last % 16"),
    ({"fc_units": 48, "feat_last": 32}, 0, b"fc_units % 32"),
    ({"fc_units": 96, "feat_last": 48}, "f16x1", b"fc_units % 64"),                        # one plane: LDS stages of 64 columns
], ids=["C17", "tau14", "tau7-ts", "H520", "H24", "W48", "W96-one-plane"])
def test_plan_refuses_heads_beyond_its_limits(kw, flags, msg):
    """make_plan refuses each head shape it cannot compute, with the named reason, and accepts the edge just inside"""
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    f = _lib.FLAG_TRAIN | (_lib.FLAG_F16X1 if flags == "f16x1" else 0)
    d = ModelSpec(**kw).desc(64, 8, f)
    assert L.snerf_packed_floats(C.byref(d)) == 0 and L.snerf_workspace_bytes(C.byref(d)) == 0
    assert msg in L.snerf_last_error(), L.snerf_last_error()
    for ok in ({"n_classes": 16}, {"t_dim": 13}, {"t_dim": 6, "use_separate_tj_for_semantic": True, "use_tj_for_s": True},
               {"feat_last": 512}, {"feat_last": 48}, {"fc_units": 96, "feat_last": 48}, {"fc_units": 1024, "feat_last": 512}):
        d = ModelSpec(**ok).desc(64, 8, _lib.FLAG_TRAIN)
        assert L.snerf_workspace_bytes(C.byref(d)) > 0, (ok, L.snerf_last_error())


def test_product_path_refuses_cpu_tensors():
    """No CPU fallback: the HIP path raises instead of computing on the host."""
    import torch
    from snerf_amd import ops
    spec = ops.ModelSpec(fc_units=32, feat_last=16)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.params_struct(spec, {n: torch.zeros(4) for n in spec.param_names()})


def test_param_names_match_reference_state_dict():
    from oracle import snerf_oracle as O
    from snerf_amd.ops import ModelSpec
    for cfg in (O.OracleCfg(), O.OracleCfg(use_separate_beta_for_s=True), O.OracleCfg(model="satnerf")):
        sem = cfg.model == "semantic"
        spec = ModelSpec(n_freq=10 if sem else 0, n_classes=5 if sem else 0,
                         use_separate_beta_for_s=cfg.use_separate_beta_for_s)
        assert spec.param_names() == list(O.param_shapes(cfg).keys())


def test_graft_entry_build_runs():
    """The driver's build check (`__graft_entry__.build()`: make for gfx950, import, ABI version): it must not lag behind the
    header (it once asserted the previous ABI version while every other test was green)."""
    import importlib
    ge = importlib.import_module("__graft_entry__")
    ge.build()
