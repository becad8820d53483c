"""k_freq past 2^32 elements with no host slab: a 4200 x 721 x 1440 int32 flag (4.36 G elements, 17.4 GB) filled on the device.
Every byte is 0x01, so every id is 16 843 009; the last 10 timesteps (all beyond element 2^32) are zeroed, and a partial block of
pixels of one timestep there.  The counts follow analytically."""
import ctypes as C

import numpy as np
import pytest

from contrack_amd import _native

pytestmark = pytest.mark.gpu

T, NY, NX = 4200, 721, 1440
ID = 0x01010101
ZERO_T = 10                        # timesteps [T - 10, T) zeroed
BLOCK_T, BLOCK_P0, BLOCK_N = 4185, 517_003, 1_001       # and pixels [BLOCK_P0, BLOCK_P0 + BLOCK_N) of timestep 4185 (odd)


def test_counts_beyond_2_32_elements():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    npix = NY * NX
    assert (T - ZERO_T) * npix > 2 ** 32 and BLOCK_T * npix > 2 ** 32
    with _native.Tracker(0) as trk:
        flag = trk.malloc(T * npix * 4)
        try:
            trk.memset(flag, 0x01, T * npix * 4)
            trk.memset(C.c_void_p(flag.value + (T - ZERO_T) * npix * 4), 0, ZERO_T * npix * 4)
            trk.memset(C.c_void_p(flag.value + (BLOCK_T * npix + BLOCK_P0) * 4), 0, BLOCK_N * 4)
            block = np.zeros(npix, dtype=bool)
            block[BLOCK_P0:BLOCK_P0 + BLOCK_N] = True

            got = trk.frequency_dev(flag, T, NY, NX).reshape(npix)
            want = np.where(block, T - ZERO_T - 1, T - ZERO_T)
            assert np.array_equal(got, want)

            ids = (np.arange(T) % 2).astype(np.int32)
            got = trk.frequency_dev(flag, T, NY, NX, group=ids, ngroups=2, above=ID - 1).reshape(2, npix)
            n_alive = (T - ZERO_T) // 2                                  # per parity among [0, 4190)
            assert np.array_equal(got[0], np.full(npix, n_alive))
            assert np.array_equal(got[1], np.where(block, n_alive - 1, n_alive))      # 4185 is odd

            assert not trk.frequency_dev(flag, T, NY, NX, above=ID).any()           # nothing above every id
        finally:
            trk.free(flag)
