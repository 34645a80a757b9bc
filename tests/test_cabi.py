"""The C-ABI library loads here (no GPU) and exports exactly what include/mfhip.h
declares; ops refuse CPU tensors instead of falling back.  No compute calls."""
import ctypes
import os
import re

import pytest
import torch

import morefusion_amd as mf
from conftest import ROOT


HEADER = os.path.join(ROOT, "include", "mfhip.h")
STRUCTS = {"mfIccBatch": mf._lib.IccBatch, "mfOccTree": mf._lib.OccTree, "mfIcpRegBatch": mf._lib.IcpRegBatch,
           "mfMeshSdfBatch": mf._lib.MeshSdfBatch}
SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "double": ctypes.c_double, "mfStream_t": ctypes.c_void_p}


def _parse_header(text):
    """-> ({function: (return type, [argument declaration, ...])}, {struct: [field declaration, ...]})"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    struct_re = r"typedef struct \{(.*?)\} (\w+);"
    structs = {name: [d.strip() for d in body.split(";") if d.strip()]
               for body, name in re.findall(struct_re, text, re.S)}
    protos = {name: (ret.strip(), [] if args.strip() in ("", "void") else [a.strip() for a in args.split(",")])
              for ret, name, args in re.findall(r"([\w\s*]+?)\b(mf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;",
                                                re.sub(struct_re, "", text, flags=re.S))}
    return protos, structs


def _ctypes_of(decl, named=True):
    """C declaration (``const float *x``, ``int32_t lo[3]``; ``named=False``: a return type) -> (name, the ctypes a
    binding may use for it).  One rule: scalars by width, every pointer ``c_void_p``, a pointer to a descriptor struct
    also ``POINTER(<its Structure>)`` (``c_void_p``: a device array of descriptors), ``const char *`` returned
    ``c_char_p``."""
    type_part, name, dim = re.fullmatch(r"(.*?)(\w+)(?:\[(\d+)\])?", decl).groups() if named else (decl, None, None)
    words = [w for w in re.findall(r"\w+|\*", type_part) if w != "const"]
    if "*" in words:
        assert words.count("*") == 1 and dim is None, decl
        if words[0] in STRUCTS:
            return name, {ctypes.POINTER(STRUCTS[words[0]]), ctypes.c_void_p}
        return name, {ctypes.c_char_p if words[0] == "char" and not named else ctypes.c_void_p}
    assert len(words) == 1 and words[0] in SCALARS, f"no rule for `{decl}`"
    return name, {SCALARS[words[0]] * int(dim) if dim else SCALARS[words[0]]}


def _abi_mismatches(header_text):
    """Every place where morefusion_amd/_lib.py (``_SIGNATURES``, the four Structures) differs from the header."""
    protos, structs = _parse_header(header_text)
    table, bad = mf._lib._SIGNATURES, []
    bad += [f"{n}: declared, not bound" for n in sorted(set(protos) - set(table))]
    bad += [f"{n}: bound, not declared" for n in sorted(set(table) - set(protos))]
    for name in sorted(set(protos) & set(table)):
        (ret, args), (argtypes, restype) = protos[name], table[name]
        if restype not in _ctypes_of(ret, named=False)[1]:
            bad.append(f"{name}: returns `{ret}`, bound as {restype.__name__}")
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments declared, {len(argtypes)} bound")
            continue
        bad += [f"{name}: argument {k} `{decl}` bound as {t.__name__}"
                for k, (decl, t) in enumerate(zip(args, argtypes)) if t not in _ctypes_of(decl)[1]]
    for cname, cls in STRUCTS.items():
        fields = [_ctypes_of(d) for d in structs[cname]]
        if [n for n, _ in fields] != [f[0] for f in cls._fields_]:
            bad.append(f"{cname}: fields {[n for n, _ in fields]} declared, {[f[0] for f in cls._fields_]} bound")
            continue
        bad += [f"{cname}.{n}: bound as {f[1].__name__}" for (n, allowed), f in zip(fields, cls._fields_)
                if f[1] not in allowed]
        size = align = 0
        for _, allowed in fields:  # natural alignment: each field at a multiple of its element size, tail padded
            t = next(iter(allowed))  # (a pointer's alternatives have one size)
            a = ctypes.sizeof(getattr(t, "_type_", t)) if hasattr(t, "_length_") else ctypes.sizeof(t)
            size, align = -(-size // a) * a + ctypes.sizeof(t), max(align, a)
        if ctypes.sizeof(cls) != -(-size // align) * align:
            bad.append(f"{cname}: {-(-size // align) * align} bytes declared, {ctypes.sizeof(cls)} bound")
    return bad


def test_library_exports_every_declared_symbol():
    lib = mf._lib.lib()  # dlopen works without a GPU
    declared = sorted(_parse_header(open(HEADER).read())[0])
    assert len(declared) >= 24
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mfhip.h but not exported"
    assert sorted(mf._lib.EXPORTED_SYMBOLS) == declared  # python binding covers the whole ABI
    assert lib.mf_version() >= 100
    assert isinstance(lib.mf_last_error_string(), bytes)


def test_binding_types_match_header():
    """Argument count, every argument type, the return type of all entry points and the layout of the four
    descriptor structs: an ``int64_t`` bound as ``int`` would not raise, it would hand a kernel a garbage size."""
    assert _abi_mismatches(open(HEADER).read()) == []


def test_binding_check_reports_a_doctored_header():
    """The comparator is not vacuous: a narrowed argument, a dropped argument and a renamed struct field are each
    reported, by name, and nothing else is."""
    text = open(HEADER).read()
    for old, new in (("const float *ref, int64_t R,", "const float *ref, int32_t R,"),
                     ("int64_t n, void *pts4,", "int64_t n,"),
                     ("double res_factor;", "double inv_resolution;")):
        assert text.count(old) == 1
        text = text.replace(old, new)
    bad = _abi_mismatches(text)
    assert len(bad) == 3, bad
    assert any(b.startswith("mf_nn: argument 1 `int32_t R`") for b in bad), bad
    assert any(b.startswith("mf_pack_points_sdf: 4 arguments declared, 5 bound") for b in bad), bad
    assert any(b.startswith("mfOccTree: fields") and "inv_resolution" in b for b in bad), bad


def test_icc_batch_struct_matches_header():
    fields = [_ctypes_of(d)[0] for d in _parse_header(open(HEADER).read())[1]["mfIccBatch"]]
    assert fields == [f[0] for f in mf._lib.IccBatch._fields_]
    assert ctypes.sizeof(mf._lib.IccBatch) == 8 * 8 + 5 * 4 + 2 * 4 + 4 + 4 + 4  # (+ flags, + tail padding to 8)


def test_workspace_size_is_host_only_arithmetic():
    def desc(n_objects, n_scenes, n_points, max_ns, thr=2.0):
        return mf._lib.IccBatch(None, None, None, None, None, None, None, None, n_objects, n_scenes,
                                n_points, 32, max_ns, thr, 0.0, 1)
    ws = mf._lib.lib().mf_icc_workspace_bytes
    n = ws(ctypes.byref(desc(8, 1, 28000, 8)))
    one = desc(8, 1, 28000, 8)
    one.flags = 1  # reserved since round 6 (round 5's opt-in one-launch iteration is gone): a set bit is refused
    assert ws(ctypes.byref(one)) < 0
    # winners of 16 grids + compact bins: per grid 68 bins of max(64, P_g / 8) records + an overflow list of 2 P_g,
    # summed over the grids (sum_g P_g = Ns * P_scene) -- O(N * sum P), not nbins x that (round 2: 68 x 8 x 28000 x 16 B)
    sumP = 8 * 28000
    assert n >= 2 * 8 * 32 ** 3 * 8 + (68 * sumP // 8 + 2 * sumP) * 16
    assert n < 2 * 8 * 32 ** 3 * 8 + 0.25 * 68 * sumP * 16
    assert ws(ctypes.byref(desc(64, 8, 8 * 28000, 8))) > n
    assert ws(ctypes.byref(desc(8, 1, 28000, 8, thr=4.0))) > n       # kernel size 5: two more planes
    assert ws(ctypes.byref(desc(40, 1, 28000, 40))) > n              # 33..64 objects in a scene: allowed since round 3
    assert ws(ctypes.byref(desc(96, 1, 28000, 96))) > n              # 65..128 objects: the single-pass path (round 6)
    assert ws(ctypes.byref(desc(130, 1, 28000, 130))) < 0            # > 128 objects in a scene
    general = desc(70, 1, 28000, 70)
    general.grid_ne_binary = 0                                       # any no-entry values: the two-kernel path stays at 64
    assert ws(ctypes.byref(general)) < 0
    assert ws(ctypes.byref(desc(8, 1, 28000, 8, thr=9.0))) < 0       # kernel size > 7


def test_ops_refuse_cpu_tensors_loudly():
    v = torch.zeros(4, 2)
    p = torch.zeros(4, 3)
    b = torch.zeros(4, dtype=torch.int32)
    # (round 5: average_voxelization_3d and occupancy_grid_3d dispatch NumPy arrays / CPU tensors to the product's own
    # CPU path, like the reference's get_array_module -- tests/test_cpu_path.py; the GPU-only ops still refuse)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mf.functions.interpolate_voxel_grid(torch.zeros(1, 1, 2, 2, 2), p, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mf.functions.truncated_distance_function(p, pitch=1.0, origin=(0, 0, 0), dims=(4, 4, 4), truncation=2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mf.geometry.nn(p, p)
    assert not mf.functions.occupancy_grid_3d(p, pitch=1.0, origin=(0, 0, 0), dims=(4, 4, 4)).is_cuda


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(mf._lib, "_lib", None)
    monkeypatch.setattr(mf._lib, "SO_PATH", str(tmp_path / "libmfhip.so"))
    with pytest.raises(RuntimeError, match="not built"):
        mf._lib.lib()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "morefusion_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("the oracle", "").replace("CPU oracle", "").replace("oracle order", "").replace("oracle)", ""), os.path.join(dp, f)


def test_wgrad_split_cost_model_is_a_host_function_with_sane_answers():
    """mf_wgrad_split (csrc/gemm_bf16.hip): no device call -- the slab count of a weight-gradient GEMM from the number
    of 128 x 128 output tiles, 64-row K-tiles and the slab size.  conv3 at the training batch (160 tiles, 1024
    K-tiles) fills exactly one round of the chip's 512 workgroup slots with 3 slabs (4 would spill a quarter-full
    second round); conv4 (512 tiles) needs none; tiny layers split deep but keep >= 8 K-tiles per slab."""
    from morefusion_amd import _lib
    L = _lib.lib()
    assert L.mf_wgrad_split(160, 1024, 256 * 10240 * 4) == 3
    assert L.mf_wgrad_split(512, 128, 512 * 16384 * 4) == 1
    assert L.mf_wgrad_split(120, 250, 1920 * 984 * 4) == 4
    for tiles, ktiles, slab in ((1, 250, 8192), (2, 8192, 6912), (7, 3, 100), (0, 0, 0), (4096, 1, 1 << 20)):
        s = L.mf_wgrad_split(tiles, ktiles, slab)
        assert 1 <= s <= 512 and (s == 1 or ktiles // s >= 8), (tiles, ktiles, s)


def test_bf16_engines_reject_operands_beyond_the_32_bit_byte_offsets():
    """the bf16 GEMM engines address operands with 32-bit BYTE offsets from a 2^31-byte buffer
    resource (an offset >= 2^31 is the masked value and reads zeros), so a tensor of 2^30 .. 2^31 ELEMENTS must be
    refused -- the old guard let it through and convolved the tail of the batch as zeros.  Host-side argument checks
    only (no launch)."""
    from morefusion_amd import _lib
    L = _lib.lib()
    # conv3 at D = 32, Cin = 160: B = 205 is the first batch beyond 2^30 input elements (204 fits)
    assert 205 * 32 ** 3 * 160 >= 1 << 30 > 204 * 32 ** 3 * 160
    assert L.mf_conv3d_bf16_fwd(None, None, None, None, 205, 160, 256, 32, 4, 2, 1, 1, 1, 0, 256, None) < 0
    assert b"2^30" in L.mf_last_error_string()
    assert L.mf_linear_bf16(None, 0, 1024, None, 0, 1024, None, 0, None, 0, 1024, 1 << 20, 1024, 1024, 1, 0, 0, 0, None) < 0
    assert b"2^31 bytes" in L.mf_last_error_string()
    assert L.mf_linear_wgrad_bf16(None, 0, 1024, None, 0, 1024, None, 0, 1024, None, 1 << 20, 1024, 1024, 1, 1, None) < 0
