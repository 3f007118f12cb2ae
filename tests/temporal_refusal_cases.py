"""The refusals of the twelve mi355pt_temporal_accumulate* entry points as one case list, shared by tools/record_temporal_refusals.py
(which writes tests/golden/temporal_refusals.json from a library) and tests/test_temporal_refusals.py (which replays it on the tree's).

A case is an entry point and one or two FAULTS put into an argument set that is valid otherwise: a 1 x 1 frame with a previous frame, a
view and half films, every buffer a real host array (16-byte aligned, all distinct), so nothing invalid is ever dereferenced and a call
that every check lets through ends in the device code, never in a crash.  The faults fall into the groups the checks run in — base,
rect (the rectify parameters), scratch (device forms), table / flow (the carry) — and a case's name says which it combines:
"base.spp_zero", "rect.null_rp+flow.null_records".  Every applicable single fault is a case; every pair of groups that apply to an entry
point gives the cases PAIR_PICKS x PAIR_PICKS, so the fixture pins which check wins.  Plain ctypes on a library path: no package."""
import ctypes as C
import itertools

import numpy as np

INVALID = -1      # MI355PT_E_INVALID
SLOT = 128        # bytes per buffer of the arena: a 1 x 1 frame's largest is one motion record (96)


class Frame(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("film", "half", "length", "position", "shading_normal", "hit")]


class View(C.Structure):
    _fields_ = [("delta", C.c_float * 3), ("rows", C.c_float * 9), ("sx", C.c_float), ("sy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class Params(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("pos_tol", "normal_cos", "min_weight", "max_history")]


class RectifyParams(C.Structure):
    _fields_ = [("radius", C.c_uint32), ("gamma", C.c_float)]


# entry point -> (carry, rectified, device form)
FORMS = {}
for _carry, _infix in ((None, ""), ("table", "_motion"), ("flow", "_flow")):
    for _rect in (False, True):
        for _device in (True, False):
            FORMS["mi355pt_temporal_accumulate" + ("_rectified" if _rect else "") + _infix + ("_device" if _device else "")] = (_carry, _rect, _device)
FRAME_KEYS = ("film", "half", "length", "position", "shading_normal", "hit")
BUFFERS = ["cur_" + k for k in FRAME_KEYS if k != "length"] + ["prev_" + k for k in FRAME_KEYS] + \
          ["out_film", "out_half", "out_length", "scratch", "ids_cur", "ids_prev", "table", "flow"]


def valid_args(arena_base):
    """the valid argument set: buffer names -> addresses in the arena, scalars, parameter tuples (None: a NULL pointer)"""
    a = {name: arena_base + SLOT * i for i, name in enumerate(BUFFERS)}
    a.update(cur=True, prev=True, view=True, cur_length=None, spp=2, width=1, height=1, tp=(0.01, 0.9, 0.01, 32.0), rp=(2, 2.0), scratch_bytes=32, n_entries=1)
    return a


def _set(**kw):
    return lambda a: a.update(kw)


def _alias(dst, src):
    return lambda a: a.update({dst: a[src]})


def _off(key):
    return lambda a: a.update({key: a[key] + 4})


def _tp(i, v):
    return lambda a: a.update(tp=a["tp"][:i] + (v,) + a["tp"][i + 1:])


# group -> [(name, edit, needs)]; needs: "" always, "device" a device form, "scratch" a rectified device form
FAULTS = {
    "base": [("null_cur", _set(cur=None), ""), ("null_tp", _set(tp=None), ""), ("null_out_film", _set(out_film=None), ""),
             ("null_out_length", _set(out_length=None), ""), ("prev_without_view", _set(view=None), ""), ("view_without_prev", _set(prev=None), ""),
             ("cur_missing_film", _set(cur_film=None), ""), ("prev_missing_length", _set(prev_length=None), ""),
             ("half_not_all", _set(out_half=None), ""), ("spp_zero", _set(spp=0), ""), ("spp_odd_with_half", _set(spp=3), ""),
             ("zero_width", _set(width=0), ""), ("frame_too_large", _set(width=(1 << 24) + 1), ""), ("nan_pos_tol", _tp(0, float("nan")), ""),
             ("max_history_half", _tp(3, 0.5), ""), ("normal_cos_two", _tp(1, 2.0), ""), ("out_is_input", _alias("out_film", "cur_film"), ""),
             ("two_equal_outputs", _alias("out_length", "out_film"), "")],
    "rect": [("null_rp", _set(rp=None), ""), ("radius_zero", _set(rp=(0, 2.0)), ""), ("radius_four", _set(rp=(4, 2.0)), ""),
             ("gamma_zero", _set(rp=(2, 0.0)), "")],
    "scratch": [("null", _set(scratch=None), ""), ("misaligned", _off("scratch"), ""), ("one_byte_short", _set(scratch_bytes=31), ""),
                ("is_output", _alias("scratch", "out_half"), "")],
    "table": [("null_ids_cur", _set(ids_cur=None), ""), ("null_table", _set(table=None), ""), ("n_entries_zero", _set(n_entries=0), ""),
              ("misaligned_table", _off("table"), "device"), ("ids_is_output", _alias("ids_prev", "out_film"), ""),
              ("table_is_output", _alias("table", "out_length"), ""), ("ids_is_scratch", _alias("ids_cur", "scratch"), "scratch"),
              ("table_is_scratch", _alias("table", "scratch"), "scratch")],
    "flow": [("null_records", _set(flow=None), ""), ("misaligned_records", _off("flow"), "device"), ("prev_ids_alone", _set(ids_cur=None), ""),
             ("records_is_output", _alias("flow", "out_half"), ""), ("ids_is_output", _alias("ids_cur", "out_length"), ""),
             ("records_is_scratch", _alias("flow", "scratch"), "scratch"), ("ids_is_scratch", _alias("ids_prev", "scratch"), "scratch")],
}
GROUP_ORDER = ["base", "rect", "scratch", "table", "flow"]
PAIR_PICKS = {"base": ["spp_zero", "out_is_input"], "rect": ["null_rp", "gamma_zero"], "scratch": ["null", "one_byte_short"],
              "table": ["n_entries_zero", "ids_is_output"], "flow": ["null_records", "ids_is_output"]}


def _groups(entry):
    carry, rect, device = FORMS[entry]
    return ["base"] + (["rect"] if rect else []) + (["scratch"] if rect and device else []) + ([carry] if carry else [])


def _applies(entry, needs):
    _, rect, device = FORMS[entry]
    return needs == "" or (needs == "device" and device) or (needs == "scratch" and rect and device)


def cases():
    """[(entry point, case name, [edit, ...])] in a fixed order"""
    out = []
    for entry in FORMS:
        groups = _groups(entry)
        table = {g: {n: e for n, e, needs in FAULTS[g] if _applies(entry, needs)} for g in groups}
        for g in groups:
            out += [(entry, "%s.%s" % (g, n), [e]) for n, e in table[g].items()]
        for g0, g1 in itertools.combinations(groups, 2):
            out += [(entry, "%s.%s+%s.%s" % (g0, n0, g1, n1), [table[g0][n0], table[g1][n1]]) for n0 in PAIR_PICKS[g0] for n1 in PAIR_PICKS[g1]]
    return out


class Caller:
    """calls the entry points of the library at `lib_path` with edited copies of the valid argument set"""

    def __init__(self, lib_path):
        self.lib = C.CDLL(lib_path)
        self.lib.mi355pt_last_error.restype = C.c_char_p
        self.arena = np.zeros(SLOT * (len(BUFFERS) + 1), np.uint8)
        self.base = (self.arena.ctypes.data + 15) & ~15

    def call(self, entry, edits):
        """-> (return code, mi355pt_last_error text)"""
        carry, rect, device = FORMS[entry]
        a = valid_args(self.base)
        for edit in edits:
            edit(a)
        frames = {k: Frame(*[a["%s_%s" % (k, f)] for f in FRAME_KEYS]) for k in ("cur", "prev")}
        view, tp = View(), Params(*a["tp"]) if a["tp"] else None
        rp = RectifyParams(*a["rp"]) if a["rp"] else None
        ref = lambda s, given=True: C.byref(s) if given and s is not None else None   # noqa: E731
        ptr, u32 = C.c_void_p, C.c_uint32
        args = [ref(frames["cur"], a["cur"]), u32(a["spp"]), ref(frames["prev"], a["prev"]), ref(view, a["view"]), u32(a["width"]), u32(a["height"]), ref(tp)]
        if rect:
            args += [ref(rp)] + ([ptr(a["scratch"]), C.c_size_t(a["scratch_bytes"])] if device else [])
        if carry:
            args += [ptr(a["ids_cur"]), ptr(a["ids_prev"])] + ([ptr(a["table"]), u32(a["n_entries"])] if carry == "table" else [ptr(a["flow"])])
        args += [ptr(a["out_film"]), ptr(a["out_half"]), ptr(a["out_length"])] + ([ptr(None)] if device else [])
        fn = getattr(self.lib, entry)
        fn.restype = C.c_int
        rc = fn(*args)
        return int(rc), (self.lib.mi355pt_last_error() or b"").decode()

    def records(self):
        return [{"entry": entry, "case": name, "code": code, "error": text}
                for entry, name, edits in cases() for code, text in [self.call(entry, edits)]]
