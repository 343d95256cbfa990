"""Guard-banded device buffers shared by the kernel-matrix runners (tests/upproj_fused_ref.py, tests/convf32_cases.py): an interior the library writes,
inside a larger allocation whose bands on each side hold a fixed bit pattern that is compared bitwise after the launch."""

GUARD = 2048                # floats on each side of an interior: 8 KiB, so 4 KiB remain where the interior starts one float later
GUARD_BITS = 0x5A5AA5A5     # (as a float: 1.5e16, finite)
_NAN_BITS, _FF_BITS = 0x7FC00000, -1                  # a quiet NaN for the outputs; 0xFF bytes (also a NaN) for the workspace


class _Guarded:
    """`n` floats, 16-byte aligned (or, `shift` = 1, one float past that), inside a larger buffer whose GUARD floats on each side hold GUARD_BITS."""

    def __init__(self, n, fill_bits, shift=0):
        import torch
        self.n, self.lo = n, GUARD + shift
        self.bits = torch.full((2 * GUARD + n + 4,), GUARD_BITS, dtype=torch.int32, device="cuda")
        assert self.bits.data_ptr() % 16 == 0
        self.bits[self.lo:self.lo + n] = fill_bits
        self.t = self.bits.view(torch.float32)[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == 4 * shift and self.t.data_ptr() == self.bits.data_ptr() + 4 * self.lo

    def guards_intact(self):
        return bool((self.bits[:self.lo] == GUARD_BITS).all().item()) and bool((self.bits[self.lo + self.n:] == GUARD_BITS).all().item())
