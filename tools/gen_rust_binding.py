#!/usr/bin/env python3
"""Generates bindings/rust/mi355pt_sys.rs — the `extern "C"` block and #[repr(C)] structs a maintainer of the reference adds — from
include/mi355pt.h and the include/mi355pt_denoise.h, include/mi355pt_adaptive.h, include/mi355pt_denoise_var.h, include/mi355pt_gbuffer.h, include/mi355pt_temporal.h, include/mi355pt_temporal_rectify.h, include/mi355pt_upsample.h, include/mi355pt_display.h, include/mi355pt_robust.h, include/mi355pt_rebase.h, include/mi355pt_instances.h, include/mi355pt_motion.h, include/mi355pt_deform.h, include/mi355pt_flow.h, include/mi355pt_budget.h, include/mi355pt_edit.h and include/mi355pt_bloom.h it includes, so that the documented Rust seam cannot drift from the header (tests/test_abi.py re-parses both and compares).
The image has no Rust toolchain: the file is generated text, checked structurally, never compiled here.
usage: tools/gen_rust_binding.py [--check]   (--check: exit 1 if the committed file differs from what the header generates)"""
import os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mi355pt.h")
DENOISE_HDR = os.path.join(ROOT, "include", "mi355pt_denoise.h")     # the denoiser block, which mi355pt.h includes
ADAPTIVE_HDR = os.path.join(ROOT, "include", "mi355pt_adaptive.h")   # the adaptive-sampling block, likewise
DENOISE_VAR_HDR = os.path.join(ROOT, "include", "mi355pt_denoise_var.h")   # the variance-guided denoiser block, likewise
GBUFFER_HDR = os.path.join(ROOT, "include", "mi355pt_gbuffer.h")   # the G-buffer block, likewise
TEMPORAL_HDR = os.path.join(ROOT, "include", "mi355pt_temporal.h")   # the temporal-reprojection block, likewise
TEMPORAL_RECTIFY_HDR = os.path.join(ROOT, "include", "mi355pt_temporal_rectify.h")   # its rectified form, likewise
UPSAMPLE_HDR = os.path.join(ROOT, "include", "mi355pt_upsample.h")   # the guided half-resolution block, likewise
DISPLAY_HDR = os.path.join(ROOT, "include", "mi355pt_display.h")   # the display block, likewise
ROBUST_HDR = os.path.join(ROOT, "include", "mi355pt_robust.h")   # the robust-film block, likewise
REBASE_HDR = os.path.join(ROOT, "include", "mi355pt_rebase.h")   # the camera-move block, likewise
INSTANCES_HDR = os.path.join(ROOT, "include", "mi355pt_instances.h")   # the instance-move block, likewise
MOTION_HDR = os.path.join(ROOT, "include", "mi355pt_motion.h")   # the object-motion block, likewise
DEFORM_HDR = os.path.join(ROOT, "include", "mi355pt_deform.h")   # the mesh-deformation block, likewise
FLOW_HDR = os.path.join(ROOT, "include", "mi355pt_flow.h")   # the per-pixel motion block, likewise
BUDGET_HDR = os.path.join(ROOT, "include", "mi355pt_budget.h")   # the sample-budget block, likewise
EDIT_HDR = os.path.join(ROOT, "include", "mi355pt_edit.h")   # the lights-and-materials block, likewise
BLOOM_HDR = os.path.join(ROOT, "include", "mi355pt_bloom.h")   # the bloom block, likewise
OUT = os.path.join(ROOT, "bindings", "rust", "mi355pt_sys.rs")

SCALARS = {"uint32_t": "u32", "int32_t": "i32", "uint64_t": "u64", "int64_t": "i64", "float": "f32", "double": "f64", "uint8_t": "u8",
           "int": "i32", "size_t": "usize", "char": "core::ffi::c_char", "void": "core::ffi::c_void"}
RUST_KEYWORDS = {"type": "ty"}


def strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def parse_header(path=HDR):
    """-> (structs: {name: [(field, ctype, array_len or None)]}, functions: [(name, ret_ctype, [(arg_name, ctype, ptr_depth, is_const)])],
    constants: [(name, value)], enums: [(name, value)])"""
    src = strip_comments(open(path).read())
    structs = {}
    for m in re.finditer(r"typedef struct (\w+) \{(.*?)\} (\w+);", src, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            ty, rest = decl.split(" ", 1)
            if ty == "const":                                                # a pointer-to-const field: the qualifier stays with the type
                ty2, rest = rest.split(" ", 1)
                ty = "const " + ty2
            for item in rest.split(","):
                item = item.strip()
                am = re.match(r"(\w+)\[(\d+)\]$", item)
                pm = re.match(r"(\*+)\s*(\w+)$", item)                       # a pointer field: the stars belong to the type
                fields.append((am.group(1), ty, int(am.group(2))) if am else (pm.group(2), ty + pm.group(1), None) if pm else (item, ty, None))
        structs[m.group(3)] = fields
    funcs = []
    for m in re.finditer(r"^\s*((?:const\s+)?\w+\s*\**)\s*(mi355pt_\w+)\s*\((.*?)\)\s*;", src, flags=re.S | re.M):
        ret = " ".join(m.group(1).split())
        args = []
        body = " ".join(m.group(3).split())
        if body and body != "void":
            for a in body.split(","):
                a = a.strip()
                const = a.startswith("const ")
                a = a[6:] if const else a
                am = re.match(r"(\w+)\s*(\**)\s*(\w+)(\[\d*\])?$", a)
                depth = len(am.group(2)) + (1 if am.group(4) else 0)
                args.append((am.group(3), am.group(1), depth, const))
        funcs.append((m.group(2), ret, args))
    consts = re.findall(r"#define (MI355PT_\w+) (\(?-?\w+\)?)\s", src)
    enums = []
    for m in re.finditer(r"enum \{(.*?)\};", src, flags=re.S):
        nxt = 0
        for item in m.group(1).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                n, v = [x.strip() for x in item.split("=")]
                nxt = int(v, 0)
            else:
                n = item
            enums.append((n, nxt))
            nxt += 1
    return structs, funcs, consts, enums


def rust_type(ctype, structs):
    if ctype.startswith("const ") and ctype.endswith("*"):
        return "*const " + rust_type(ctype[6:-1], structs)
    if ctype.endswith("*"):
        return "*mut " + rust_type(ctype[:-1], structs)
    if ctype in SCALARS:
        return SCALARS[ctype]
    if ctype in structs or ctype == "mi355pt_scene":
        return rust_struct_name(ctype)
    raise ValueError(ctype)


def rust_struct_name(cname):
    return "".join(p.capitalize() for p in cname.replace("mi355pt_", "").split("_"))


def generate():
    structs, funcs, consts, enums = parse_header()
    for hdr in (DENOISE_HDR, ADAPTIVE_HDR, DENOISE_VAR_HDR, GBUFFER_HDR, TEMPORAL_HDR, TEMPORAL_RECTIFY_HDR, UPSAMPLE_HDR, DISPLAY_HDR, ROBUST_HDR, REBASE_HDR, INSTANCES_HDR, MOTION_HDR, DEFORM_HDR, FLOW_HDR, BUDGET_HDR, EDIT_HDR, BLOOM_HDR):   # what a caller of mi355pt.h sees: all eighteen headers
        for part, more in zip((structs, funcs, consts, enums), parse_header(hdr)):
            part.update(more) if isinstance(part, dict) else part.extend(more)
    o = ["// GENERATED by tools/gen_rust_binding.py from include/mi355pt.h (+ mi355pt_denoise.h, mi355pt_adaptive.h, mi355pt_denoise_var.h, mi355pt_gbuffer.h, mi355pt_temporal.h, mi355pt_temporal_rectify.h, mi355pt_upsample.h, mi355pt_display.h, mi355pt_robust.h, mi355pt_rebase.h, mi355pt_instances.h, mi355pt_motion.h, mi355pt_deform.h, mi355pt_flow.h, mi355pt_budget.h, mi355pt_edit.h, mi355pt_bloom.h) — do not edit; `tools/gen_rust_binding.py --check` and",
         "// tests/test_abi.py::test_rust_binding_matches_header keep it in step with the header.",
         "// The seam: renderer/src/renderer.rs:120-134 (RendererImage::render) calls mi355pt_render instead of the rayon pixel loop.",
         "#![allow(dead_code, non_upper_case_globals)]", ""]
    for n, v in consts:
        v = v.strip("()")
        v = v[:-1] if v.startswith("0x") and v.endswith("u") else v
        o.append(f"pub const {n}: {'u32' if v.startswith('0x') else 'i32'} = {v};")
    for n, v in enums:
        o.append(f"pub const {n}: u32 = {v};")
    o += ["", "#[repr(C)] pub struct Scene { _private: [u8; 0] }   // opaque mi355pt_scene", ""]
    for name, fields in structs.items():
        o.append("#[repr(C)] #[derive(Clone, Copy)]")
        o.append(f"pub struct {rust_struct_name(name)} {{")
        for f, ty, n in fields:
            rt = rust_type(ty, structs)
            o.append(f"    pub {RUST_KEYWORDS.get(f, f)}: {f'[{rt}; {n}]' if n else rt},")
        o.append("}")
        o.append("")
    o.append('#[link(name = "mi355pt")]')
    o.append('extern "C" {')
    for name, ret, args in funcs:
        ra = []
        for an, ty, depth, const in args:
            rt = rust_type(ty, structs)
            for _ in range(depth):
                rt = ("*const " if const else "*mut ") + rt
            ra.append(f"{RUST_KEYWORDS.get(an, an)}: {rt}")
        rr = ""
        if ret != "void":
            cm = re.match(r"(const\s+)?(\w+)\s*(\**)", ret)
            rt = rust_type(cm.group(2), structs)
            for _ in cm.group(3):
                rt = ("*const " if cm.group(1) else "*mut ") + rt
            rr = f" -> {rt}"
        o.append(f"    pub fn {name}({', '.join(ra)}){rr};")
    o.append("}")
    return "\n".join(o) + "\n"


if __name__ == "__main__":
    text = generate()
    if "--check" in sys.argv:
        sys.exit(0 if os.path.exists(OUT) and open(OUT).read() == text else 1)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").write(text)
    print("wrote", OUT)
