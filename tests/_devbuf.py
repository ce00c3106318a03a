"""Device memory for tests, from the HIP runtime the engine uses (ctypes; the DeviceBuf of
test_gpu_slice_window.py with a fill and an offset pointer)."""
import ctypes

import numpy as np


class DeviceBuf:
    def __init__(self, n, fill=None):
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.p = ctypes.c_void_p()
        self.n = n
        assert self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(n)) == 0
        assert self.p.value % 256 == 0
        if fill is not None:
            self.fill(fill)

    def fill(self, byte):
        """Every byte set, and the device idle after it (the engine's streams do not wait for
        the null stream)."""
        assert self.hip.hipMemset(self.p, ctypes.c_int(byte), ctypes.c_size_t(self.n)) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def at(self, off):
        assert 0 <= off < self.n
        return self.p.value + off

    def host(self):
        h = np.empty(self.n, np.uint8)
        assert self.hip.hipMemcpy(ctypes.c_void_p(h.ctypes.data), self.p, ctypes.c_size_t(self.n), 2) == 0
        return h

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = ctypes.c_void_p()
