"""A guarded, poisoned, exactly sized workspace for the launches of `sigsvgd_amd.ops` (tests/test_gpu_workspace.py).

`ops._launch` asks `ops._workspace(dev, nbytes)` for the buffer of every launch that has a `*_workspace_bytes` query and
passes the tensor's `data_ptr()` and the returned size on to the library.  The cached buffer `ops` keeps is a quarter larger
than the query, 256-B aligned, and holds what the launch before left in it.  `GuardedWorkspace` stands in for that function
(`install(monkeypatch)`) and gives every request one allocation of its own,

    [front guard | offset | interior of exactly nbytes | back guard]

of which the library sees the interior alone: exactly the queried bytes, at an address the caller chooses modulo 256, filled
with what the caller chooses.  The guards belong to the same allocation, so a kernel that writes outside its plan writes
memory the test owns; `check()` finds the bytes it changed.  Plain torch, no device code: tests/test_support.py runs it on
CPU tensors."""
import torch

MIN_GUARD = 1 << 20
FILLS = ("zeros", "ones", "random")


class GuardedWorkspace:
    """The replacement for `ops._workspace(dev, nbytes) -> (tensor, numel)`.

    fill: the interior before the launch -- "zeros"; "ones": every byte 0xFF (a NaN as fp32 and fp64, all ones as a
    counter); "random": seeded bytes, plausible finite numbers among them.
    offset: 0 or 1, the interior's address modulo 256.  At 1 the library's 256-B aligned base lies 255 B in: all of the
    alignment slack a plan's total carries is used up, the worst case the contract allows.
    short: the size reported to the library is nbytes - short, the allocation keeps the full layout.
    Guards: at least 1 MiB in front, at least max(1 MiB, nbytes // 4 + 4096) behind (everything the slack of the cached
    buffer can hide), filled from a seeded byte generator -- a kernel's stray zeros or 0xFF do not pass for an intact guard.
    Every buffer stays alive until `check()`, which synchronises, compares the guards with their copies and forgets them."""

    def __init__(self, fill="zeros", offset=0, short=0, seed=20240607):
        assert fill in FILLS and offset in (0, 1) and short >= 0
        self.fill, self.offset, self.short, self.seed = fill, offset, short, seed
        self.requests = []  # of this test, in order; check() empties it
        self.count = 0      # workspace requests so far (nbytes == 0 included)
        self.sizes = []     # nbytes of every request so far, kept across check()

    def install(self, monkeypatch):
        from sigsvgd_amd import ops

        monkeypatch.setattr(ops, "_workspace", self)
        return self

    @staticmethod
    def back_guard_bytes(nbytes):
        return max(MIN_GUARD, nbytes // 4 + 4096)

    def _bytes(self, n, dev, k, what):
        g = torch.Generator(device=dev)
        g.manual_seed(self.seed + 4 * k + what)
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=g)

    def _filled(self, n, dev, k):
        if self.fill == "random":
            return self._bytes(n, dev, k, 2)
        return torch.full((n,), 0 if self.fill == "zeros" else 0xFF, dtype=torch.uint8, device=dev)

    def __call__(self, dev, nbytes):
        self.count += 1
        self.sizes.append(int(nbytes))
        if nbytes == 0:
            return None, 0
        k = self.count
        buf = torch.empty(MIN_GUARD + 256 + 1 + nbytes + self.back_guard_bytes(nbytes), dtype=torch.uint8, device=dev)
        front = MIN_GUARD + (-(buf.data_ptr() + MIN_GUARD)) % 256  # the interior at offset 0 starts on a multiple of 256
        start = front + self.offset
        back = buf.numel() - start - nbytes  # the back guard runs to the allocation's end
        guards = (self._bytes(start, dev, k, 0), self._bytes(back, dev, k, 1))  # (the offset byte is front guard too)
        buf[:start] = guards[0]
        buf[start:start + nbytes] = self._filled(nbytes, dev, k)
        buf[start + nbytes:start + nbytes + back] = guards[1]
        interior = buf[start:start + nbytes]
        assert interior.data_ptr() % 256 == self.offset
        self.requests.append(dict(k=k, nbytes=nbytes, buf=buf, front=front, start=start, back=back, guards=guards))
        return interior, nbytes - self.short

    def interior(self, i=-1):
        """the interior of the i-th live request (what the library was given, at its full size)"""
        r = self.requests[i]
        return r["buf"][r["start"]:r["start"] + r["nbytes"]]

    def interior_untouched(self, i=-1):
        """whether the interior of the i-th live request still holds its fill"""
        r = self.requests[i]
        return torch.equal(self.interior(i), self._filled(r["nbytes"], r["buf"].device, r["k"]))

    def failures(self):
        """One line per damaged guard of the live requests.  Offsets of the front guard are relative to the interior's first
        byte (negative), those of the back guard to the interior's end (0 = the first byte behind it)."""
        out = []
        for r in self.requests:
            buf, start, n = r["buf"], r["start"], r["nbytes"]
            if buf.device.type == "cuda":
                torch.cuda.synchronize(buf.device)
            end = start + n
            for name, got, want, origin in (("front", buf[:start], r["guards"][0], -start),
                                            ("back", buf[end:end + r["back"]], r["guards"][1], 0)):
                if torch.equal(got, want):
                    continue
                bad = torch.nonzero(got != want).flatten()
                out.append(f"workspace request {r['k']} of the test (nbytes={n}, offset {self.offset}, fill {self.fill}): "
                           f"{name} guard changed in {bad.numel()} bytes, lowest at {int(bad[0]) + origin:+d}, highest at "
                           f"{int(bad[-1]) + origin:+d} relative to the interior's {'start' if name == 'front' else 'end'}")
        return out

    def check(self):
        """Synchronise and compare both guards of every live request with their copies; AssertionError names the request and
        the lowest and highest changed byte.  The buffers are released."""
        bad = self.failures()
        self.requests = []
        assert not bad, "\n".join(bad)
