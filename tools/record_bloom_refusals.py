#!/usr/bin/env python3
"""Writes tests/golden/bloom_refusals.json: the refusals of mi355pt_bloom_device / mi355pt_bloom (include/mi355pt_bloom.h) as data.  A case
is ONE fault put into a call that is valid otherwise — an 8 x 4 frame of spp 4, two levels, every buffer at its own offset of one 16-byte
aligned arena — together with the verdict csrc/bloom_checks.hpp must give; nothing here asks a library.  tests/test_bloom.py replays every
case through the library's entry points and through the predicate's check program (tests/bloom_checks_check.cpp).
Buffers are OFFSETS into the arena (null: a NULL pointer); the params' floats are u32 bit patterns, since JSON has no NaN.
usage: tools/record_bloom_refusals.py"""
import json
import os
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "bloom_refusals.json")
W, H, SPP, LEVELS = 8, 4, 4, 2
FILM_BYTES = W * H * 12
NEED = 16 * (4 * 2 + 2 * 1)
VALID = dict(film=0, out=512, scratch=1024, record=1536, scratch_bytes=NEED, width=W, height=H, spp=SPP)
ARENA_BYTES = 2048
FLOATS = ("threshold", "knee", "scatter", "base", "intensity", "exposure")
PARAMS = dict(levels=LEVELS, firefly=1, threshold=0.0, knee=0.5, scatter=0.7, base=0.96, intensity=0.04, exposure=1.0)


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def case(name, verdict, forms="both", params=PARAMS, **edits):
    c = dict(name=name, verdict=verdict, forms=forms, **VALID)
    c.update(edits)
    c["params"] = None if params is None else {k: (f32_bits(v) if k in FLOATS else v) for k, v in params.items()}
    return c


def with_field(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


def cases():
    nan, inf = float("nan"), float("inf")
    out = [case("null.params", "NULL_POINTER", params=None), case("null.film", "NULL_POINTER", film=None), case("null.out", "NULL_POINTER", out=None),
           case("null.scratch", "NULL_POINTER", forms="device", scratch=None),
           case("spp.zero", "SPP_ZERO", spp=0),
           case("frame.zero_width", "EMPTY_FRAME", width=0), case("frame.zero_height", "EMPTY_FRAME", height=0),
           case("frame.width_above_2^24", "FRAME_TOO_LARGE", width=(1 << 24) + 1, height=1), case("frame.height_above_2^24", "FRAME_TOO_LARGE", width=1, height=(1 << 24) + 1),
           case("frame.2^32_pixels", "FRAME_TOO_LARGE", width=1 << 16, height=1 << 16), case("frame.2^24x2^8", "FRAME_TOO_LARGE", width=1 << 24, height=1 << 8),
           case("scratch.one_byte_short", "SCRATCH_TOO_SMALL", forms="device", scratch_bytes=NEED - 1), case("scratch.zero_bytes", "SCRATCH_TOO_SMALL", forms="device", scratch_bytes=0),
           case("scratch.sized_for_one_level", "SCRATCH_TOO_SMALL", forms="device", scratch_bytes=16 * 8),
           case("align.scratch+4", "MISALIGNED", forms="device", scratch=1024 + 4, scratch_bytes=NEED + 16), case("align.scratch+8", "MISALIGNED", forms="device", scratch=1024 + 8),
           case("align.record+2", "MISALIGNED", record=1536 + 2), case("align.record+1", "MISALIGNED", record=1536 + 1),
           case("params.zeroed", "LEVELS", params={k: 0 if k in ("levels", "firefly") else 0.0 for k in PARAMS})]
    bad = dict(levels=("LEVELS", (0, 9, 0xffffffff)), firefly=("FIREFLY", (2, 0xffffffff)), threshold=("THRESHOLD", (-1.0, 65536.5, inf, nan, -inf)),
               knee=("KNEE", (-0.01, 1.01, nan, inf)), scatter=("SCATTER", (-0.5, 1.5, nan)), base=("BASE", (-0.1, 1.1, nan, inf)),
               intensity=("INTENSITY", (-0.04, 16.5, nan, inf)), exposure=("EXPOSURE", (0.0, -1.0, inf, nan)))
    for field, (verdict, values) in bad.items():
        out += [case("params.%s=%r" % (field, v), verdict, params=with_field(**{field: v})) for v in values]
    out += [case("overlap.out_in_film+4", "OVERLAP", out=4), case("overlap.out_last_word_of_film", "OVERLAP", out=FILM_BYTES - 4),
            case("overlap.film_in_out", "OVERLAP", film=512 + 12), case("overlap.record_in_film", "OVERLAP", record=16), case("overlap.record_in_out", "OVERLAP", record=512 + FILM_BYTES - 4),
            case("overlap.scratch_is_film", "OVERLAP", forms="device", scratch=0), case("overlap.scratch_in_out", "OVERLAP", forms="device", scratch=512 + 16),
            case("overlap.record_in_scratch", "OVERLAP", forms="device", record=1024 + NEED - 4), case("overlap.scratch_end_in_out", "OVERLAP", forms="device", film=1536 + 64, out=1024 + NEED - 16, record=None),
            # which check wins
            case("order.null_before_spp", "NULL_POINTER", film=None, spp=0), case("order.spp_before_frame", "SPP_ZERO", spp=0, width=0),
            case("order.frame_before_params", "FRAME_TOO_LARGE", width=1 << 16, height=1 << 16, params=with_field(levels=0)),
            case("order.params_before_scratch", "KNEE", forms="device", params=with_field(knee=2.0), scratch_bytes=0),
            case("order.levels_before_firefly", "LEVELS", params=with_field(levels=9, firefly=2)),
            case("order.small_before_misaligned", "SCRATCH_TOO_SMALL", forms="device", scratch=1024 + 4, scratch_bytes=NEED - 16),
            case("order.misaligned_before_overlap", "MISALIGNED", record=17)]
    # calls that every check lets through
    out += [case("ok.valid", "OK"), case("ok.in_place", "OK", out=0), case("ok.no_record", "OK", record=None), case("ok.eight_levels", "OK", params=with_field(levels=8), scratch_bytes=16 * (8 + 2 + 6)),
            case("ok.edges_of_every_range", "OK", params=with_field(levels=1, firefly=0, threshold=65536.0, knee=1.0, scatter=0.0, base=0.0, intensity=16.0, exposure=1e-30)),
            case("ok.scratch_larger", "OK", forms="device", scratch_bytes=NEED + 100)]
    return out


if __name__ == "__main__":
    doc = dict(about="the refusals of mi355pt_bloom_device / mi355pt_bloom: tools/record_bloom_refusals.py", arena_bytes=ARENA_BYTES, cases=cases())
    assert len({c["name"] for c in doc["cases"]}) == len(doc["cases"])
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, len(doc["cases"]), "cases")
