"""The table behind tests/test_list_checks.py and tools/record_list_checks.py: a deterministic list of calls to the
three ore_image_check*_oriented entries and their non-oriented forms, built to pin the ORDER of the rules and the TEXT
of every message (the ABI tests match substrings and seldom break two rules at once).

Per format: a valid descriptor; every rule broken alone, at index 0 and at index 2 of 3; every two consecutive rules
of the format's order broken together; orientations null, all 1, transposing, and the bad codes 0 and 9; the filters
0, 1, 256, 257 and an unknown one; n of 0 and -1; null imgs; bad output shapes.  No pointer is ever dereferenced.

cases() -> [(name, call)], call(L) -> [status, bad_index, ore_last_error(NULL)].  The recording
(tests/golden/list_check_messages.json) was made by the library as it stood before the three checks became one."""
import ctypes

from ore import _lib

FAKE = 0x1000  # a non-null pointer that is never dereferenced
H, W = 5, 7    # the lists' output shape
BIG = 120000000  # a stride at which 20 rows (or 10) reach past 2^31 bytes
FILTERS = {"bilinear": 0, "aa": 1, "bicubic": 256, "bicubic_aa": 257}


def _base(fmt):
    """A valid 20 x 30 descriptor resized to 10 x 14, window at (1, 2); yuv: an I420 frame."""
    d = {"hs": 20, "ws": 30, "g": [10, 14, 1, 2]}
    if fmt == "u8":
        d.update(data=FAKE, row_stride=0)
    elif fmt == "nv12":
        d.update(y=FAKE, uv=FAKE, y_stride=0, uv_stride=0)
    else:
        d.update(plane=[FAKE, FAKE, FAKE], stride=[0, 0, 0], format=_lib.YUV_FORMATS["i420"], reserved=0)
    return d


def _gray():
    d = _base("yuv")
    d.update(plane=[FAKE, 0, 0], format=_lib.YUV_FORMATS["gray"])
    return d


def _with(d, **kw):
    """d with fields replaced; g_rh .. g_left and plane0 .. stride2 address the arrays' elements."""
    d = {k: (list(v) if isinstance(v, list) else v) for k, v in d.items()}
    for k, v in kw.items():
        if k.startswith("g_"):
            d["g"][("rh", "rw", "top", "left").index(k[2:])] = v
        elif k[:-1] in ("plane", "stride") and k[-1].isdigit():
            d[k[:-1]][int(k[-1])] = v
        else:
            assert k in d, k
            d[k] = v
    return d


# The rules of one descriptor in the order the checks try them: (rule, fields that break it and nothing earlier).
# The orientation rule comes first everywhere and is broken through the codes, not through a field.
RULES = {
    "u8": [
        ("null", dict(data=0)),
        ("range", dict(hs=0)),
        ("crop", dict(g_top=6)),
        ("stride", dict(row_stride=89)),
        ("reach", dict(row_stride=BIG)),
        ("ratio", dict(hs=400)),
    ],
    "nv12": [
        ("null", dict(y=0)),
        ("range", dict(ws=16385)),
        ("crop", dict(g_left=8)),
        ("ystride", dict(y_stride=29)),
        ("uvstride", dict(uv_stride=29)),
        ("yreach", dict(y_stride=BIG)),
        ("uvreach", dict(uv_stride=2 * BIG)),
        ("ratio", dict(ws=600)),
    ],
    "yuv": [
        ("format", dict(format=8)),
        ("reserved", dict(reserved=3)),
        ("plane0", dict(plane0=0)),
        ("plane1", dict(plane1=0)),
        ("plane2", dict(plane2=0)),
        ("range", dict(g_rh=0)),
        ("crop", dict(g_top=-1)),
        ("stride0", dict(stride0=29)),
        ("stride1", dict(stride1=14)),
        ("stride2", dict(stride2=-4)),
        ("reach0", dict(stride0=BIG)),
        ("reach1", dict(stride1=2 * BIG)),
        ("reach2", dict(stride2=1 << 31)),
        ("ratio", dict(hs=400)),
    ],
}
# Two consecutive rules that one field cannot break both ways (a stride below its row and past 2^31): a negative stride
PAIRS = {
    "u8": {("stride", "reach"): dict(row_stride=-5)},
    "nv12": {("uvstride", "yreach"): dict(uv_stride=29, y_stride=BIG), ("ystride", "uvstride"): dict(y_stride=29, uv_stride=29),
             ("yreach", "uvreach"): dict(y_stride=BIG, uv_stride=2 * BIG)},
    "yuv": {("stride2", "reach0"): dict(stride2=-4, stride0=BIG), ("stride0", "stride1"): dict(stride0=29, stride1=14),
            ("stride1", "stride2"): dict(stride1=14, stride2=-4), ("reach0", "reach1"): dict(stride0=BIG, stride1=2 * BIG),
            ("reach1", "reach2"): dict(stride1=2 * BIG, stride2=1 << 31)},
}
# Further descriptors, each alone at index 1 of 3: the other spellings of a message and the edges of a rule
EXTRA = {
    "u8": [
        ("range_hs_max", dict(hs=16385)), ("range_rw", dict(g_rw=0)), ("range_rh_max", dict(g_rh=16385)),
        ("crop_left", dict(g_left=8)), ("crop_negative", dict(g_top=-1)), ("stride_exact", dict(row_stride=90)),
        ("stride_negative", dict(row_stride=-5)), ("reach_stride_2g", dict(row_stride=1 << 31)),
        ("reach_one_row", dict(hs=1, row_stride=1 << 31, g_rh=5, g_top=0)), ("ratio_columns", dict(ws=600)),
        ("ratio_edge", dict(hs=320)), ("ratio_cubic_edge", dict(hs=161)),
    ],
    "nv12": [
        ("null_uv", dict(uv=0)), ("null_both", dict(y=0, uv=0)), ("range_hs", dict(hs=0)), ("crop_top", dict(g_top=6)),
        ("odd_dense", dict(hs=19, ws=29)), ("odd_uvstride", dict(ws=29, uv_stride=29)), ("odd_uvstride_ok", dict(ws=29, uv_stride=30)),
        ("uvreach_two_rows", dict(hs=3, uv_stride=1 << 31, g_rh=5, g_top=0)), ("uvreach_one_row", dict(hs=2, uv_stride=1 << 31, g_rh=5, g_top=0)),
        ("ratio_rows", dict(hs=400)),
    ],
    "yuv": [
        ("format_negative", dict(format=-1)), ("reserved_negative", dict(reserved=-1)), ("range_ws", dict(ws=0)),
        ("crop_left", dict(g_left=8)), ("ratio_columns", dict(ws=600)),
        ("nv12_third_plane", dict(format=0)), ("nv12", dict(format=0, plane2=0)), ("nv12_uvstride", dict(format=0, plane2=0, stride1=29)),
        ("nv12_stride2_unused", dict(format=0, plane2=0, stride2=-4)),
        ("yuyv", dict(format=1, plane1=0, plane2=0)), ("yuyv_stride", dict(format=1, plane1=0, plane2=0, stride0=59)),
        ("yuyv_odd", dict(format=1, plane1=0, plane2=0, ws=29, stride0=60)), ("yuyv_second_plane", dict(format=1, plane2=0)),
        ("i444_stride", dict(format=2, stride1=29)), ("i440_reach", dict(format=3, stride2=2 * BIG)), ("i422_stride", dict(format=4, stride2=14)),
        ("i411_stride", dict(format=6, stride1=7)), ("i411_ok", dict(format=6, stride1=8, stride2=8)),
        ("gray_second_plane", dict(format=7, plane2=0)), ("gray_third_plane", dict(format=7, plane1=0)),
        ("gray_both_planes", dict(format=7)), ("gray", dict(format=7, plane1=0, plane2=0)),
        ("gray_null", dict(format=7, plane0=0, plane1=0, plane2=0)),
    ],
}

_STRUCT = {"u8": _lib.ImageU8, "nv12": _lib.ImageNv12, "yuv": _lib.ImageYuv}


def _array(fmt, descs):
    arr = (_STRUCT[fmt] * max(len(descs), 1))()
    for r, d in zip(arr, descs):
        for k, v in d.items():
            if k == "g":
                r.g = _lib.Resize(*v)
            elif k in ("plane", "stride"):
                for j, x in enumerate(v):
                    getattr(r, k)[j] = x
            else:
                setattr(r, k, v)
    return arr


def _call(fmt, descs, n=None, codes=None, filt=1, c=3, hw=(H, W), entry="oriented", null_imgs=False, no_bad=False):
    """One call: entry "oriented" (codes: None for a null array), "ex" (the non-oriented form with a filter) or
    "plain" (ore_image_check, interleaved only)."""
    n = len(descs) if n is None else n

    def run(L):
        arr = None if null_imgs else _array(fmt, descs)
        bad = ctypes.c_int64(-1)
        b = None if no_bad else ctypes.byref(bad)
        cs = None if codes is None else (ctypes.c_uint8 * max(len(codes), 1))(*codes)
        lead = (arr, n, c) if fmt == "u8" else (arr, n)
        if entry == "oriented":
            fn = {"u8": L.ore_image_check_oriented, "nv12": L.ore_image_check_nv12_oriented, "yuv": L.ore_image_check_yuv_oriented}[fmt]
            st = fn(*lead, hw[0], hw[1], filt, cs, b)
        elif entry == "ex":
            fn = {"u8": L.ore_image_check_ex, "nv12": L.ore_image_check_nv12, "yuv": L.ore_image_check_yuv}[fmt]
            st = fn(*lead, hw[0], hw[1], filt, b)
        else:
            st = L.ore_image_check(*lead, hw[0], hw[1], b)
        msg = L.ore_last_error(None)
        return [int(st), int(bad.value), (msg or b"").decode()]
    return run


def _at(fmt, d, index, n=3):
    return [d if i == index else _base(fmt) for i in range(n)]


def cases():
    out = []

    def add(name, call):
        assert all(name != k for k, _ in out), name
        out.append((name, call))

    # one successful call first, so that the message of a passing call below is this library's last failure
    for fmt in ("u8", "nv12", "yuv"):
        base, rules = _base(fmt), RULES[fmt]
        add(f"{fmt}/prime", _call(fmt, [base], filt=2))
        add(f"{fmt}/valid", _call(fmt, [base] * 3))
        for entry in ("ex",) + (("plain",) if fmt == "u8" else ()):
            add(f"{fmt}/valid/{entry}", _call(fmt, [base] * 3, entry=entry))
        # orientations: null (above), all 1, transposing, mixed, and the bad codes, with and without a bad geometry behind
        add(f"{fmt}/codes/ones", _call(fmt, [base] * 3, codes=[1, 1, 1]))
        for code in range(2, 9):
            add(f"{fmt}/codes/all{code}", _call(fmt, [base] * 3, codes=[code] * 3))
        add(f"{fmt}/codes/mixed", _call(fmt, [base] * 3, codes=[1, 6, 3]))
        for code in (0, 9):
            for index in (0, 2):
                codes = [6, 6, 6]
                codes[index] = code
                add(f"{fmt}/codes/bad{code}@{index}", _call(fmt, [base] * 3, codes=codes))
            first = rules[0]
            add(f"{fmt}/codes/bad{code}+{first[0]}", _call(fmt, _at(fmt, _with(base, **first[1]), 1), codes=[1, code, 1]))
        add(f"{fmt}/codes/bad_beyond_n", _call(fmt, [base] * 3, n=2, codes=[1, 8, 0]))
        add(f"{fmt}/codes/no_bad_index", _call(fmt, [base] * 3, codes=[1, 9, 1], no_bad=True))
        # every rule alone: at index 0 and at index 2 of 3, under a transposing code, and through the non-oriented entry
        for rule, fields in rules:
            d = _with(base, **fields)
            add(f"{fmt}/{rule}@0", _call(fmt, _at(fmt, d, 0)))
            add(f"{fmt}/{rule}@2", _call(fmt, _at(fmt, d, 2)))
            add(f"{fmt}/{rule}@0/code6", _call(fmt, _at(fmt, d, 0), codes=[6, 1, 1]))
            add(f"{fmt}/{rule}@2/ex", _call(fmt, _at(fmt, d, 2), entry="ex"))
        if fmt == "u8":
            for rule, fields in rules:
                add(f"u8/{rule}@1/plain", _call(fmt, _at(fmt, _with(base, **fields), 1), entry="plain"))
        # every two consecutive rules together
        for (ra, fa), (rb, fb) in zip(rules, rules[1:]):
            fields = PAIRS[fmt].get((ra, rb), {**fa, **fb})
            add(f"{fmt}/{ra}+{rb}", _call(fmt, _at(fmt, _with(base, **fields), 1)))
        # two bad descriptors: the first is named
        add(f"{fmt}/two_bad", _call(fmt, [base, _with(base, **rules[-1][1]), _with(base, **rules[0][1])]))
        add(f"{fmt}/no_bad_index", _call(fmt, _at(fmt, _with(base, **rules[1][1]), 1), no_bad=True))
        for name, fields in EXTRA[fmt]:
            add(f"{fmt}/{name}", _call(fmt, _at(fmt, _with(base, **fields), 1)))
        # the ratio rule under each filter (32 times, 16 times, none), on stored axes under a transposing code
        ratio = _with(base, hs=400, ws=600)
        for fname, filt in FILTERS.items():
            add(f"{fmt}/filter/{fname}/valid", _call(fmt, [base], filt=filt))
            add(f"{fmt}/filter/{fname}/ratio", _call(fmt, [ratio], filt=filt))
            add(f"{fmt}/filter/{fname}/ratio/code6", _call(fmt, [ratio], filt=filt, codes=[6]))
            add(f"{fmt}/filter/{fname}/ratio/ex", _call(fmt, [ratio], filt=filt, entry="ex"))
            add(f"{fmt}/filter/{fname}/rows_240", _call(fmt, [_with(base, hs=240)], filt=filt))
        # the rules of the whole call, in their order: filter, count, output shape, n == 0, null imgs
        bad = _with(base, **rules[0][1])
        for filt in (2, -1, 255, 258, 512):
            add(f"{fmt}/filter/unknown{filt}", _call(fmt, [base], filt=filt))
        add(f"{fmt}/filter/unknown/ex", _call(fmt, [base], filt=3, entry="ex"))
        add(f"{fmt}/filter+count", _call(fmt, [base], n=-1, filt=2))
        add(f"{fmt}/count", _call(fmt, [base], n=-1))
        add(f"{fmt}/count/ex", _call(fmt, [base], n=-1, entry="ex"))
        add(f"{fmt}/count+shape", _call(fmt, [base], n=-1, hw=(0, W)))
        for hw in ((0, W), (H, 0), (-1, W), (1 << 31, 1), (1 << 16, 1 << 15), (1 << 15, 1 << 15)):
            add(f"{fmt}/shape/{hw[0]}x{hw[1]}", _call(fmt, [base], hw=hw))
        add(f"{fmt}/shape/ex", _call(fmt, [base], hw=(H, 0), entry="ex"))
        add(f"{fmt}/shape+empty", _call(fmt, [base], n=0, hw=(0, 0)))
        add(f"{fmt}/shape+null", _call(fmt, [base], hw=(0, 0), null_imgs=True))
        add(f"{fmt}/empty", _call(fmt, [bad], n=0))
        add(f"{fmt}/empty/null", _call(fmt, [], n=0, null_imgs=True))
        add(f"{fmt}/empty/bad_code", _call(fmt, [bad], n=0, codes=[0]))
        add(f"{fmt}/empty/ex", _call(fmt, [], n=0, null_imgs=True, entry="ex"))
        add(f"{fmt}/null", _call(fmt, [], n=3, null_imgs=True))
        add(f"{fmt}/null/codes", _call(fmt, [], n=1, null_imgs=True, codes=[0]))
        add(f"{fmt}/null/ex", _call(fmt, [], n=1, null_imgs=True, entry="ex"))
    # the interleaved list's channel count: judged with the output shape
    u8 = _base("u8")
    for c in (0, 1, 2, 4, 5, -3):
        add(f"u8/channels/{c}", _call("u8", [u8], c=c))
    add("u8/channels/1/stride", _call("u8", [_with(u8, row_stride=29)], c=1))
    add("u8/channels/4/stride", _call("u8", [_with(u8, row_stride=119)], c=4))
    add("u8/channels+shape", _call("u8", [u8], c=5, hw=(0, 0)))
    add("u8/channels/plain", _call("u8", [u8], c=5, entry="plain"))
    add("u8/count+channels", _call("u8", [u8], n=-1, c=0))
    return out
