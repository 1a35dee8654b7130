"""The C-ABI library loads and exports every symbol include/gsplat_hip.h declares (no compute
calls: runs without a GPU)."""
import ctypes
import os
import re

from gaussian_splatting_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_boundary():
    names = declared_symbols()
    # one entry point per function of src/bindings.cpp:118-159 (get_sorted_gaussian_list is split
    # in two; the two render entries take the reference's own argument lists, their _packed forms the
    # record of gs_pack_splats)
    for n in ["gs_camera_projection", "gs_camera_projection_backward", "gs_compute_sigma_world",
              "gs_compute_sigma_world_backward", "gs_compute_projection_jacobian",
              "gs_compute_projection_jacobian_backward", "gs_compute_conic", "gs_compute_conic_backward",
              "gs_precompute_rgb_from_sh", "gs_precompute_rgb_from_sh_backward", "gs_tile_count", "gs_tile_workspace_ints",
              "gs_preprocess_forward", "gs_preprocess_backward",
              "gs_tile_emit_sort", "gs_pack_splats", "gs_render_tiles", "gs_render_tiles_backward",
              "gs_render_tiles_packed", "gs_render_tiles_backward_packed",
              "gs_render_depth", "gs_last_error", "gs_abi_version"]:
        assert n in names


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_hip.LIB_PATH), "build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')"
    lib = ctypes.CDLL(_hip.LIB_PATH)
    missing = [n for n in declared_symbols() if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.gs_abi_version() >= 1


def test_python_loader_lists_the_same_symbols():
    assert sorted(_hip.EXPORTS) == declared_symbols()
    # EXPORTS is what the loader's parser found in the header: one prototype per declared symbol, none missed
    protos, _ = _hip.parse_header(open(_hip.HEADER_PATH).read())
    assert os.path.samefile(_hip.HEADER_PATH, os.path.join(ROOT, "include", "gsplat_hip.h"))
    assert sorted(protos) == declared_symbols()


def test_loader_applies_the_headers_prototypes():
    """_hip.lib() types every entry point from include/gsplat_hip.h: spot checks of the exact argtypes / restype"""
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p
    lib = _hip.lib()
    for name in declared_symbols():
        assert getattr(lib, name).argtypes is not None, name
    P = c_void_p

    def proto(name):
        fn = getattr(lib, name)
        return fn.restype, list(fn.argtypes)

    assert proto("gs_abi_version") == (c_int, [])
    assert proto("gs_last_error") == (c_char_p, [])
    assert proto("gs_cut_workspace_ints") == (c_size_t, [c_int, c_int])
    assert proto("gs_tile_emit_sort") == (c_int, [P, P, P, c_int, P, P, P, c_int, c_int, c_float, c_int, c_int, P, P, P,
                                                  c_int64, P, c_int, P])
    assert proto("gs_preprocess_backward_adam") == (
        c_int, [P, c_int, P, P, P, P, P, P, c_int, c_int, P] + [P, P, P, c_double, c_int64] * 5 + [c_double] * 3 + [P])
    assert proto("gs_stream_copy") == (c_int, [P, P, c_size_t, c_int, P])
    assert proto("gs_adam_step") == (c_int, [c_int] + [P] * 7 + [c_double] * 3 + [P])


def test_header_parser_refuses_types_it_does_not_know():
    """the parser maps the header's scalar types by name and never guesses: an unknown one is an error that names the
    function (header texts as strings; nothing is written next to the real header)"""
    import pytest
    protos, defines = _hip.parse_header("/* c */ #define GS_A (-3)\n#define GS_B 7 // d\nsize_t gs_f(const void* p, int64_t n /*[n]*/,\n  float x);")
    assert protos == {"gs_f": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_float])}
    assert defines == {"GS_A": -3, "GS_B": 7}
    for text, name in (("int gs_good(int a);\nint gs_bad_long(const void* p, long x, void* stream);", "gs_bad_long"),
                       ("int gs_bad_unsigned(unsigned n);", "gs_bad_unsigned"),
                       ("int gs_bad_unsigned_int(int a, unsigned int n);", "gs_bad_unsigned_int"),
                       ("long gs_bad_return(void);", "gs_bad_return"),
                       ("struct gs_s gs_bad_struct(int a);", "gs_bad_struct")):
        with pytest.raises(_hip.HipLibraryError, match=name):
            _hip.parse_header(text)


def test_typed_calls_convert_nothing_silently():
    """on the built library, no GPU needed: a float where the header says int is an error, a size_t return is whole without
    any restype set by the caller, and the constants are the header's"""
    import pytest
    lib = _hip.lib()
    with pytest.raises(ctypes.ArgumentError):
        lib.gs_cut_supported(82.5, 0, 53, 1)
    w = lib.gs_cut_workspace_ints(2_860_000, 4346)
    assert w >= 2_860_000 + 2_860_000 // 2 + 256 * 1024 + 2 * 4346
    lib.gs_cut_workspace_ints.restype = ctypes.c_size_t    # what callers once had to remember
    assert lib.gs_cut_workspace_ints(2_860_000, 4346) == w
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name, value in (("GS_SORT_PREFIX", 1024), ("GS_CUT_HIST_BINS", 8192), ("GS_F32", 0), ("GS_F64", 1),
                        ("GS_BACKWARD_DEFAULT", -1), ("GS_BACKWARD_COMPAT", 0), ("GS_BACKWARD_EXACT", 1)):
        assert getattr(_hip, name) == value, name
        assert re.search(r"#define %s \(?%d\)?\s" % (name, value), src), name
    # and _hip.py holds no copy of them
    own = open(os.path.join(ROOT, "gaussian_splatting_amd", "_hip.py")).read()
    assert not re.search(r"^GS_[A-Z0-9_]+\s*=", own, flags=re.M)


def test_native_splat_cuda_module_exports_the_reference_names():
    """csrc/bindings_hip.cpp: the compiled `splat_cuda` module has the 14 functions of
    src/bindings.cpp:118-159 and raises RuntimeError (TORCH_CHECK) for a non-device tensor"""
    import pytest
    import torch

    from gaussian_splatting_amd import splat_cuda, splat_cuda_native
    mod = splat_cuda_native.load()
    names = ["render_tiles_cuda", "render_tiles_backward_cuda", "camera_projection_cuda",
             "camera_projection_backward_cuda", "compute_sigma_world_cuda", "compute_sigma_world_backward_cuda",
             "compute_projection_jacobian_cuda", "compute_projection_jacobian_backward_cuda", "compute_conic_cuda",
             "compute_conic_backward_cuda", "get_sorted_gaussian_list", "precompute_rgb_from_sh_cuda",
             "precompute_rgb_from_sh_backward_cuda", "render_depth_cuda"]
    for n in names:
        assert callable(getattr(mod, n)) and callable(getattr(splat_cuda, n)), n
    with pytest.raises(RuntimeError, match="xyz is not a CUDA tensor"):
        mod.camera_projection_cuda(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(3, 2))
    splat_cuda_native.install("splat_cuda_test_alias")
    import sys
    assert sys.modules.pop("splat_cuda_test_alias") is mod


def test_library_shares_the_hip_runtime_torch_loaded():
    """loading the library before `import torch` must not bring a second libamdhip64 into the process
    (the second runtime to initialise finds no device: __graft_entry__.build() followed by smoke())"""
    import subprocess
    import sys
    code = ("from gaussian_splatting_amd import _hip\n_hip.lib()\nimport torch\n"
            "print(len({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "1", out.stdout


def _prototypes():
    """{function name: [declared type of each parameter, "*" for any pointer]} of include/gsplat_hip.h"""
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gs_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        params = m.group(2).strip()
        out[m.group(1)] = [] if params in ("", "void") else ["*" if "*" in p else p.split()[0] for p in params.split(",")]
    return out


# the ctypes constructor that may wrap an argument of each declared type
_WRAPPER = {"*": "c_void_p", "int": "c_int", "float": "c_float", "double": "c_double", "int64_t": "c_int64",
            "size_t": "c_size_t"}


def test_python_call_sites_pass_as_many_arguments_as_the_header_declares():
    """ctypes calls carry no prototype: a call site that drifts from include/gsplat_hip.h would corrupt the
    arguments silently.  Every `_hip.call("gs_...", ...)` / `lib.gs_...(...)` in the package, bench.py and the
    scripts must pass exactly the declared number of arguments, and an argument written as a `ctypes.c_X(...)`
    constructor must be of the parameter's declared type (the loader's prototypes raise on the others at run time;
    this finds them without running the call)."""
    import ast
    protos = _prototypes()
    assert len(protos) == len(declared_symbols()) and protos["gs_abi_version"] == []
    assert protos["gs_camera_projection"] == ["*", "*", "int", "*", "int", "*"]
    assert set(t for types in protos.values() for t in types) == set(_WRAPPER)
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for d in ("gaussian_splatting_amd", "scripts", "tests"):
        files += [os.path.join(ROOT, d, f) for f in sorted(os.listdir(os.path.join(ROOT, d))) if f.endswith(".py")]
    checked, wrappers, bad = 0, 0, []
    for path in files:
        tree = ast.parse(open(path).read())
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            name, n_args, args = None, None, []
            f = node.func
            if isinstance(f, ast.Attribute) and f.attr == "call" and node.args and isinstance(node.args[0], ast.Constant) \
                    and isinstance(node.args[0].value, str) and node.args[0].value.startswith("gs_"):
                name, n_args, args = node.args[0].value, len(node.args) - 1, node.args[1:]   # _hip.call("gs_x", a, b, ...)
            elif isinstance(f, ast.Attribute) and f.attr.startswith("gs_") and f.attr in protos:
                name, n_args, args = f.attr, len(node.args), node.args                    # lib.gs_x(a, b, ...)
            if name is None or any(isinstance(a, ast.Starred) for a in node.args):
                continue
            checked += 1
            if name not in protos or len(protos[name]) != n_args:
                bad.append((os.path.relpath(path, ROOT), node.lineno, name, n_args, protos.get(name)))
                continue
            for i, (a, declared) in enumerate(zip(args, protos[name])):
                if isinstance(a, ast.Call) and isinstance(a.func, ast.Attribute) and isinstance(a.func.value, ast.Name) \
                        and a.func.value.id == "ctypes" and a.func.attr.startswith("c_"):
                    wrappers += 1
                    if a.func.attr != _WRAPPER[declared]:
                        bad.append((os.path.relpath(path, ROOT), a.lineno, name, i, a.func.attr, declared))
    assert checked >= 40, checked
    assert wrappers >= 10, wrappers    # the tests and scripts keep theirs
    assert not bad, bad


def test_package_passes_plain_values_to_the_typed_abi():
    """the loader's argtypes do the conversion: outside _hip.py the package constructs no scalar / pointer wrapper by
    hand (ctypes ARRAYS, `(ctypes.c_int32 * n)(...)`, are data and stay)"""
    pkg = os.path.join(ROOT, "gaussian_splatting_amd")
    hits = []
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py") and f != "_hip.py":
            for i, line in enumerate(open(os.path.join(pkg, f)), 1):
                if re.search(r"\bctypes\.c_(float|double|int64|void_p)\(", line):
                    hits.append(f"{f}:{i}")
    assert not hits, hits


def test_product_sources_carry_no_experiment_builds():
    """timing-only emulations and A/B switches live in scripts/experiments/*.patch, not in the shipping translation
    units (round-5 review): no GS_EMU_* token and none of the retired A/B macros in csrc/ or include/"""
    banned = re.compile(r"GS_EMU_|GS_CK_NOREC|GS_CK_NOEPI|GS_XCD_SEG|GS_ARITH_FAST|GS_BWD_RCP_REFINE|"
                        r"GS_PRIV_XCD|GS_EMIT_NOSTORE|GS_EMIT_CELL|GS_CUT_EMIT_PREFETCH|GS_CUT_GENERAL_SORT")
    hits = []
    for d in (os.path.join(ROOT, "gaussian_splatting_amd", "csrc"), os.path.join(ROOT, "include")):
        for name in sorted(os.listdir(d)):
            if name.endswith((".hip", ".h", ".cpp")) or name == "Makefile":
                for i, line in enumerate(open(os.path.join(d, name), errors="replace"), 1):
                    if banned.search(line):
                        hits.append(f"{name}:{i}")
    assert not hits, hits
