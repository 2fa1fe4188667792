"""Device memory for a test to hand a context as its dense table (Context.adopt_dense_table), so
that the test decides what the table holds before a solve."""
import ctypes

from gamesmanmpi_amd import _lib

# Fill byte of the sweeps: the 1-byte code of LOSS in 127 (csrc/gm_common.hpp), which no position
# of up to 8 heaps has (remoteness <= 120), so a stale byte, a row or a box that a solve skipped
# cannot equal an expected code
POISON = 0x80


class _Table:
    """Device memory (4 GiB unless told otherwise) from the HIP runtime the library has loaded (no
    second framework in the test process)."""

    def __init__(self, nbytes=1 << 32):
        _lib.lib()
        path = [l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l][0]
        self.hip = ctypes.CDLL(path)
        for f, args in (("hipMalloc", [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]),
                        ("hipMemset", [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]),
                        ("hipFree", [ctypes.c_void_p]), ("hipDeviceSynchronize", [])):
            getattr(self.hip, f).argtypes = args
            getattr(self.hip, f).restype = ctypes.c_int
        self.nbytes = nbytes
        self.ptr = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.ptr), nbytes) == 0

    def data_ptr(self):
        return self.ptr.value

    def numel(self):
        return self.nbytes

    def fill(self, byte):
        assert self.hip.hipMemset(self.ptr, byte, self.nbytes) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def free(self):
        assert self.hip.hipFree(self.ptr) == 0
