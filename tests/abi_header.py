"""What the header tests of the map entries share (tests/test_*_cpu.py): one extension header of include/ against its group of rows in
_lib.HEADER_SIGNATURES, as tests/test_abi_cpu.py compares the main header with the main table.  A helper, not a test module."""
import os
import re

from snerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The symbols of every extension header, frozen at ABI 6, in the order the headers were added.  A new header adds its line here; no
# older line changes.
FROZEN = {
    "snerf_orthorect.h": ["snerf_orthorectify"],
    "snerf_raycast.h": ["snerf_dsm_segment_hit"],
    "snerf_fuse.h": ["snerf_fuse_count", "snerf_fuse_scatter", "snerf_fuse_select"],
    "snerf_objects.h": ["snerf_objects_link", "snerf_objects_stats"],
    "snerf_terrain.h": ["snerf_terrain_workspace_bytes", "snerf_terrain_keys", "snerf_terrain_open", "snerf_terrain_fill"],
    "snerf_roofs.h": ["snerf_roofs_normals", "snerf_roofs_link", "snerf_roofs_moments", "snerf_roofs_residuals"],
    "snerf_solar.h": ["snerf_solar_horizon", "snerf_solar_svf", "snerf_solar_irradiate"],
    "snerf_normals.h": ["snerf_normals_scratch_bytes", "snerf_density_grad", "snerf_test_normals_grid", "snerf_test_normals_dump"],
}


def check_header(header, names, returns=None):
    """include/<header> against _lib.HEADER_SIGNATURES[header].  `names`: symbol -> parameter names, in the header's order;
    `returns`: symbol -> return type in _c_type's terms where it is not int.
      - every prototype has a row and the reverse, in the header's order; parameter names, return type, parameter count and, per
        parameter, class, width and signedness; the stream marker exactly where the parameter is called `stream`;
      - lib() applied the row, call() knows the symbol; it is in neither the main table nor the rows of any other header;
      - the main header names nothing of this one (its file stem, symbols, structs, constant prefixes) and is included by it;
      - every header's symbols are the frozen ones, and the ABI version is 6."""
    from tests.test_abi_cpu import _c_type, _table_type
    text = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", src, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(snerf_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        protos[name] = (_c_type(ret), [(_c_type(t), n) for t, n in (re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(","))])
    assert {h: list(rows) for h, rows in _lib.HEADER_SIGNATURES.items()} == FROZEN and list(_lib.HEADER_SIGNATURES) == list(FROZEN)
    rows = _lib.HEADER_SIGNATURES[header]
    assert list(rows) == list(protos) == list(names) == FROZEN[header]
    for symbol, (ret, params) in protos.items():
        restype, argtypes = rows[symbol]
        assert _table_type(restype) == ret == (returns or {}).get(symbol, ("int", 4, True)), (symbol, restype, ret)
        assert len(argtypes) == len(params) and [n for _, n in params] == list(names[symbol]), (symbol, params)
        for k, (t, (want, pname)) in enumerate(zip(argtypes, params)):
            got = _table_type(t)
            assert got == want or (want[0] == "pointer" and got == ("pointer", None)), (symbol, k, pname, t, want)
            assert (t is _lib.c_stream) == (pname == "stream"), (symbol, k, pname)
        fn = getattr(_lib.lib(), symbol)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes) and symbol in _lib._PLANS
        assert symbol not in _lib.SIGNATURES and symbol not in _lib.EXPORTED_SYMBOLS
        assert all(symbol not in other for h, other in _lib.HEADER_SIGNATURES.items() if h != header)
    main = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    own = [header[:-2]] + list(protos) + re.findall(r"\} (\w+);", text) + re.findall(r"^#define (SNERF_[A-Z0-9]+_)", text, flags=re.M)
    assert len(own) >= 3 and not [word for word in own if word in main], [word for word in own if word in main]
    assert '#include "snerf_hip.h"' in text
    assert _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
