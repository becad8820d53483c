"""Which scalar threshold kernel a launch picks: a restatement of ctk_threshold_form in contrack_amd/csrc/ctk_forms.h (the rows per
workgroup rbt, the float4 test v4, the ballot form v6, the loads per lane u7), which launch_threshold in ctk_api.hip maps to the
kernel instance, so that the tests can choose shapes that reach every form.  Host-only; kept in step with the C++ by
tests/test_threshold_forms.py, which compares it with the library itself (ctk_debug_forms), and, on the GPU, by a kernel trace of tests/test_gpu_threshold_scalar.py."""

CTK_RB = 16                                      # rows per workgroup of the streaming kernels (ctk_device.h)
FORMS = ("v7_4", "v7_5", "v7_6", "v7_7", "v7_8", "v6", "generic_f32", "generic_f64")


def threshold_form(T, ny, nx, f64, aligned):
    """'v7_<U>' (k_threshold_v7<OP, U>), 'v6' (k_threshold_v6), 'generic_f32' / 'generic_f64' (k_threshold<OP, float / double>) for
    a launch over T steps of a (ny, nx) grid; aligned: the slab's device address is a multiple of 16 bytes"""
    W = (nx + 63) // 64
    rbt = min(ny, CTK_RB)
    nblk4 = T * ((ny + rbt - 1) // rbt)
    v4 = not f64 and nx % 4 == 0 and aligned and nblk4 < (1 << 24)
    if not f64 and W <= 64 and not v4:
        return "v6"
    if f64:
        return "generic_f64"
    if not v4:
        return "generic_f32"
    L = (min(rbt, ny) * W * 16 + 255) // 256
    best, u7 = 1 << 30, 8
    for u in range(8, 3, -1):
        waste = (L + u - 1) // u * u - L
        if waste < best:
            best, u7 = waste, u
    return "v7_%d" % u7


# (T, ny, nx, aligned) of the mask tests.  ny % 16 != 0 leaves a partial last 16-row workgroup, nx % 64 != 0 a partial last mask word.
F32_SHAPES = [
    (8, 61, 72, True),           # v7_4
    (8, 13, 360, True),          # v7_5 (ny < 16: one workgroup of 13 rows per step)
    (4, 181, 360, True),         # v7_6
    (8, 9, 1440, True),          # v7_7
    (8, 33, 1440, True),         # v7_8 (as (721, 1440): 16 full rows of 23 words per workgroup)
    (8, 17, 65, True),           # v6: nx % 4 != 0
    (8, 7, 64, False),           # v6: a slab that is not 16-byte aligned
    (6, 5, 4097, True),          # generic float32: nx % 4 != 0 and W > 64
    (4, 3, 4161, True),          # generic float32
    (4, 19, 4200, False),        # generic float32: not 16-byte aligned, W > 64
]
F64_SHAPES = [(8, 61, 72, True), (6, 17, 65, True), (4, 5, 4097, True), (4, 19, 4200, False)]
# (T, ny, nx) of the streamed mask tests (float32 forms of a whole-slab launch: v7_4, v6, generic_f32)
STREAM_SHAPES = [(7, 61, 72), (7, 17, 65), (5, 3, 4161)]
