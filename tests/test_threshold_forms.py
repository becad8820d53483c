"""The shapes of tests/test_gpu_threshold_scalar.py reach every scalar threshold kernel (tests/threshold_forms.py restates the
selection, ctk_threshold_form in ctk_forms.h, and is compared here with what the library itself decides: ctk_debug_forms).  No GPU needed."""
import threshold_forms as tf


def test_issue_examples_pick_the_stated_loads_per_lane():
    assert [tf.threshold_form(4, ny, nx, False, True) for ny, nx in ((61, 72), (13, 360), (181, 360), (9, 1440), (721, 1440))] == \
        ["v7_4", "v7_5", "v7_6", "v7_7", "v7_8"]


def test_rule_edges():
    assert tf.threshold_form(3, 7, 4096, False, False) == "v6"               # W = 64: still the ballot form
    assert tf.threshold_form(3, 7, 4100, False, False) == "generic_f32"      # W = 65
    assert tf.threshold_form(3, 7, 4100, False, True) != "generic_f32"       # aligned and nx % 4 == 0: v7
    assert tf.threshold_form(3, 7, 64, True, True) == "generic_f64"
    assert tf.threshold_form((1 << 24) // 2, 31, 64, False, True) == "v6"     # 2^24 workgroups: past the v7 grid limit


def test_mask_test_shapes_cover_every_form():
    got = {tf.threshold_form(T, ny, nx, False, al) for T, ny, nx, al in tf.F32_SHAPES}
    got |= {tf.threshold_form(T, ny, nx, True, al) for T, ny, nx, al in tf.F64_SHAPES}
    assert got == set(tf.FORMS)
    assert {tf.threshold_form(T, ny, nx, False, True) for T, ny, nx in tf.STREAM_SHAPES} == {"v7_4", "v6", "generic_f32"}
    for T, ny, nx, _ in tf.F32_SHAPES + tf.F64_SHAPES:                    # partial 16-row groups and partial last words are in
        assert T >= 2
    assert any(ny % 16 and tf.threshold_form(T, ny, nx, False, al).startswith("v7") for T, ny, nx, al in tf.F32_SHAPES)
    assert all(nx % 64 for _, _, nx, _ in tf.F32_SHAPES if nx != 64)


# ---- the restatement against the library's own rule (ctk_threshold_form in contrack_amd/csrc/ctk_forms.h, through ctk_debug_forms) ----
def _lib_form(T, ny, nx, f64, aligned, field=False):
    from contrack_amd import _native
    p = _native.forms(T, ny, nx, f64=f64, aligned16=aligned, field=field)
    assert p["thr_rbt"] == min(ny, tf.CTK_RB)
    return {0: "v7_%d" % p["thr_u7"], 1: "v6", 2: "generic_f32", 3: "generic_f64", 4: "field_vec", 5: "field_gen"}[p["thr_kind"]]


def test_restatement_agrees_with_the_library():
    shapes = [(T, ny, nx) for T, ny, nx, _ in tf.F32_SHAPES + tf.F64_SHAPES] + list(tf.STREAM_SHAPES)
    # both sides of every edge of the rule: nx % 4, W = 64 / 65, a partial last workgroup, 2^24 workgroups of 16 rows
    shapes += [(T, ny, nx) for T in (1, 512, 513) for ny in (1, 15, 16, 17, 181, 721) for nx in (4, 63, 64, 360, 1440, 4092, 4096, 4097, 4100, 4160)]
    shapes += [(T, ny, 64) for ny in (16, 17, 31, 32, 33) for T in ((1 << 24) // ((ny + 15) // 16) + d for d in (-1, 0, 1))]
    n = 0
    for T, ny, nx in shapes:
        for f64 in (False, True):
            for aligned in (False, True):
                assert _lib_form(T, ny, nx, f64, aligned) == tf.threshold_form(T, ny, nx, f64, aligned), (T, ny, nx, f64, aligned)
                # the field kernels take the float4 test alone
                v4 = tf.threshold_form(T, ny, nx, f64, aligned).startswith("v7")
                assert _lib_form(T, ny, nx, f64, aligned, field=True) == ("field_vec" if v4 else "field_gen")
                n += 1
    assert n > 800
