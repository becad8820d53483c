"""The binding is derived from the headers (contrack_amd/_abi.py): the parser on header text given here, one declaration of every
tricky kind and the declarations it must refuse; then what it makes of the real headers against the loaded library, with the sizes and
offsets of the structs as literal numbers.  Host only: the library is loaded, no compute call is made."""
import ctypes as C
import os
import re

import pytest

from contrack_amd import _abi, _native

P, I, I64 = C.c_void_p, C.c_int, C.c_int64

TEXT = """
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define CTK_OK         0
#define CTK_E_THING   -9   /* a comment that
                              runs on, with int ctk_not_a_function(int n); inside */
#define CTK_RATIO      1.5
typedef struct ctk_handle ctk_handle;
typedef struct ctk_pair {
    int32_t a, b;                   /* two to a line */
    const double *p, *q;
    uint32_t *n; float f;
    uint64_t gen;
} ctk_pair;
typedef int (*ctk_cb_fn)(void *user, int64_t t0, const int32_t *src);
int ctk_a(const void *const *blobs, void **out, const char *name);
const char *ctk_b(void);
void *ctk_c(ctk_handle *h);
double ctk_d(const double *a, size_t n);
void   ctk_e(ctk_handle *h, uint64_t seed, uint32_t k, float f);
int ctk_f(ctk_handle *h, ctk_cb_fn cb, void *user, const ctk_pair *pair);
int ctk_g(ctk_handle *h /* the handle; (not) a type, */, int n /* [n], ... */);
int ctk_h(ctk_handle *h,
          int64_t T,
          double q);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_each_tricky_kind():
    abi = _abi.parse(TEXT)
    assert abi.functions == {
        "ctk_a": (I, [P, P, C.c_char_p]),                           # const void *const *, void **, const char *
        "ctk_b": (C.c_char_p, []),                                  # const char * return, (void)
        "ctk_c": (P, [P]),                                          # void * return, an opaque handle
        "ctk_d": (C.c_double, [P, C.c_size_t]),
        "ctk_e": (None, [P, C.c_uint64, C.c_uint32, C.c_float]),    # void return
        "ctk_f": (I, [P, abi.callbacks["ctk_cb_fn"], P, P]),        # a callback, a pointer to a struct
        "ctk_g": (I, [P, I]),                                       # comments inside the argument list
        "ctk_h": (I, [P, I64, C.c_double]),                         # three lines
    }
    assert list(abi.functions) == ["ctk_a", "ctk_b", "ctk_c", "ctk_d", "ctk_e", "ctk_f", "ctk_g", "ctk_h"]      # the header's order
    assert list(abi.callbacks) == ["ctk_cb_fn"] and abi.callbacks["ctk_cb_fn"] is C.CFUNCTYPE(I, P, I64, P)
    assert abi.structs == {"ctk_pair": [("a", C.c_int32), ("b", C.c_int32), ("p", P), ("q", P), ("n", P), ("f", C.c_float), ("gen", C.c_uint64)]}
    assert abi.constants == {"CTK_OK": 0, "CTK_E_THING": -9}        # integers only


@pytest.mark.parametrize("decl, named", [
    ("int ctk_bad_type(ctk_handle *h, long n);", "ctk_bad_type"),
    ("int ctk_bad_pointee(ctk_other *o);", "ctk_bad_pointee"),
    ("int ctk_bad_words(unsigned int n);", "ctk_bad_words"),
    ("int ctk_bad_value(ctk_handle *h, ctk_pair pair);", "ctk_bad_value"),
    ("int ctk_bad_handle(ctk_handle h);", "ctk_bad_handle"),
    ("int ctk_bad_variadic(const char *fmt, ...);", "ctk_bad_variadic"),
    ("int ctk_bad_array(int v[4]);", "ctk_bad_array"),
    ("long ctk_bad_return(void);", "ctk_bad_return"),
    ("int ctk_bad_tail(int n) __attribute__((cold));", "ctk_bad_tail"),
    ("typedef long (*ctk_bad_fn)(void *user);", "ctk_bad_fn"),
    ("typedef struct ctk_bad_struct { int v[4]; } ctk_bad_struct;", "ctk_bad_struct"),
    ("typedef struct ctk_bad_field { ctk_pair inner; } ctk_bad_field;", "ctk_bad_field"),
])
def test_parser_fails_closed(decl, named):
    with pytest.raises(_abi.AbiError, match=named):
        _abi.parse(TEXT.replace("int ctk_h(", decl + "\nint ctk_h("))


# ---- the real headers ---------------------------------------------------------------------------------------------------------
ABI = _native.ABI


def test_every_declared_function_is_exported_and_bound_as_declared():
    lib = _native.lib()
    assert _native.EXPORTS == list(ABI.functions) and len(_native.EXPORTS) >= 202
    text = re.sub(r"/\*.*?\*/", "", "".join(open(os.path.join(_native.INCLUDE_DIR, h)).read() for h in _abi.HEADERS), flags=re.S)
    for name, (restype, argtypes) in ABI.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
        args, = re.findall(r"\b%s\s*\(([^()]*)\)\s*;" % name, text)                  # counted by another route: the commas
        assert len(fn.argtypes) == (0 if args.strip() == "void" else args.count(",") + 1), name
    want = dict(ctk_last_error=C.c_char_p, ctk_comm_rccl_library=C.c_char_p, ctk_destroy=None, ctk_result_free=None, ctk_comm_group_destroy=None,
                ctk_comm_destroy=None, ctk_debug_np_sum=C.c_double, ctk_stream=P)
    assert {n: r for n, (r, _) in ABI.functions.items() if r is not I} == want
    assert ABI.functions["ctk_comm_init_shm"][1] == [P, C.c_char_p, I, I, P]         # a str must be refused, not passed as wchar_t *
    with pytest.raises(C.ArgumentError):
        lib.ctk_comm_init_shm(None, "name", 0, 1, None)


def test_f32_f64_twins_have_equal_signatures():
    twins = 0
    for name in ABI.functions:
        if "_f64" in name:
            twin = name.replace("_f64", "_f32") if name.replace("_f64", "_f32") in ABI.functions else name.replace("_f64", "")
            assert ABI.functions[twin] == ABI.functions[name], name
            twins += 1
    assert twins >= 27 and twins == sum("_f32" in n for n in ABI.functions) + 1     # + ctk_shard_label2d, the one without a suffix


def test_host_entries_end_in_chunk_steps_where_dev_entries_end_in_a_flag():
    """pairs that differ in the width of their last argument only: a slip here shows beyond 2^31 alone"""
    pairs = {}
    for name, (_, argtypes) in ABI.functions.items():
        if name.endswith("_dev") and argtypes[-1] is I:
            host = ABI.functions[name[:-4]][1]
            assert host[-1] is I64 and host[:-1] == argtypes[:-1], name
            pairs[name] = name[:-4]
    assert sorted(pairs) == ["ctk_centred_f32_dev", "ctk_centred_f64_dev", "ctk_composite_f32_dev", "ctk_composite_f64_dev", "ctk_frequency_dev"]


def test_callback_types():
    cb = ABI.callbacks
    assert sorted(cb) == ["ctk_life_pick_fn", "ctk_read_chunk_fn", "ctk_write_chunk_fn", "ctk_write_values_fn"]
    assert cb["ctk_write_chunk_fn"] is cb["ctk_write_values_fn"] is _native.WRITE_CHUNK_FN         # one signature, one ctypes class
    assert _native.READ_CHUNK_FN is cb["ctk_read_chunk_fn"] is C.CFUNCTYPE(I, P, I64, I64, P)
    assert _native.LIFE_PICK_FN is cb["ctk_life_pick_fn"] is C.CFUNCTYPE(I, P, P, I64, P, P)
    assert ABI.functions["ctk_anom_stream_cb"][1][5] is _native.READ_CHUNK_FN and ABI.functions["ctk_anom_stream_cb"][1][15] is _native.WRITE_CHUNK_FN


def _layout(struct):
    return C.sizeof(struct), [(n, getattr(struct, n).offset, C.sizeof(t)) for n, t in struct._fields_]


def test_struct_layouts():
    assert _layout(_native.BandSpec) == (48, [("y0", 0, 4), ("y1", 4, 4), ("above", 8, 4), ("nsect", 12, 4), ("w", 16, 8), ("sectors", 24, 8),
                                              ("columns", 32, 4), ("resident", 36, 4), ("resident_gen", 40, 8)])
    assert _layout(_native.BandOut) == (48, [(n, 8 * i, 8) for i, n in enumerate("cnt area wx sec_cnt sec_area sec_wx".split())])
    size, fields = _layout(_native.FormQuery)
    assert size == 176 and [f[1:] for f in fields] == [(8 * i, 8) for i in range(22)]
    assert [f[0] for f in fields][:5] == ["T", "nt", "ny", "nx", "f64"] and fields[-1][0] == "launched"
    size, fields = _layout(_native.FormPlan)
    assert size == 336 and [f[1:] for f in fields] == [(8 * i, 8) for i in range(42)]
    assert fields[0][0] == "thr_kind" and fields[-1][0] == "rowcount_groups"
    assert all(t is I64 for _, t in _native.FormQuery._fields_ + _native.FormPlan._fields_)


def test_record_dtypes():
    d = _native.LIFE_ROW
    assert d.itemsize == 48 and [(n, d.fields[n][0].str, d.fields[n][1]) for n in d.names] == [
        ("t", "<i4", 0), ("label", "<i4", 4), ("shift", "<i4", 8), ("pad", "<i4", 12), ("area", "<f8", 16), ("swv", "<f8", 24), ("swvy", "<f8", 32),
        ("swvx", "<f8", 40)]
    d = _native.LIFE_EXACT
    assert d.itemsize == 40 and [(n, d.fields[n][0].str, d.fields[n][1]) for n in d.names] == [
        ("area", "<f8", 0), ("swv", "<f8", 8), ("s", "<f8", 16), ("sy", "<f8", 24), ("sx", "<f8", 32)]


def test_constants():
    k = ABI.constants
    assert k["CTK_NSTATS"] == 25 and k["CTK_NTIMERS"] == len(_native.TIMER_NAMES)
    assert (k["CTK_OK"], k["CTK_E_INVALID"], k["CTK_E_NOMEM"], k["CTK_E_RANGE"], k["CTK_E_COMM"]) == (0, -1, -3, -4, -7)
    assert (_native.CTK_E_INVALID, _native.CTK_E_NOMEM, _native.CTK_E_RANGE, _native.CTK_E_COMM) == (-1, -3, -4, -7)


def test_check_maps_the_codes_to_the_same_exceptions():
    for rc, exc in ((-1, ValueError), (-4, ValueError), (-3, MemoryError), (-7, _native.CommError), (-2, _native.ContrackHipError),
                    (-5, _native.ContrackHipError), (-6, _native.ContrackHipError)):
        with pytest.raises(exc) as e:
            _native.check(rc)
        assert type(e.value) is exc
    assert _native.check(0) is None


def test_a_declared_function_the_library_lacks_is_one_error_with_every_name(monkeypatch):
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "ABI", ABI._replace(functions=dict(ABI.functions, ctk_not_there=(I, []), ctk_nor_this=(I, [P]))))
    with pytest.raises(_native.ContrackHipError, match="ctk_not_there, ctk_nor_this"):
        _native.lib()


def test_missing_headers_are_a_contrack_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, "INCLUDE_DIR", str(tmp_path))
    with pytest.raises(_native.ContrackHipError, match="CTK_INCLUDE"):
        _native._headers()
