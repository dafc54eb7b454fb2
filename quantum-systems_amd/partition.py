"""The contiguous split of an index over the ranks: shared by the ``torch.distributed`` layer (sharded.py) and the
C ABI's communicator (``kernels.RcclComm``)."""


class SlabPartition:
    """Contiguous split of ``n`` rows over ``world`` ranks: balanced by default, or the explicit
    ``starts`` (world + 1 non-decreasing offsets from 0 to n) -- spin doubling turns the balanced split of
    l spatial rows into twice those offsets, which is not the balanced split of 2l when l % world != 0."""

    def __init__(self, n, world, starts=None):
        if world < 1 or n < 1:
            raise ValueError("need n >= 1 and world >= 1")
        self.n, self.world = int(n), int(world)
        if starts is None:
            base, extra = divmod(self.n, self.world)
            self.starts = [r * base + min(r, extra) for r in range(self.world + 1)]
        else:
            self.starts = [int(x) for x in starts]
            if (len(self.starts) != self.world + 1 or self.starts[0] != 0 or self.starts[-1] != self.n
                    or any(b < a for a, b in zip(self.starts, self.starts[1:]))):
                raise ValueError(f"bad partition {self.starts} of {self.n} rows over {self.world} ranks")

    def bounds(self, rank):
        return self.starts[rank], self.starts[rank + 1]

    def count(self, rank):
        lo, hi = self.bounds(rank)
        return hi - lo

    def doubled(self):
        """The partition of the 2n spin rows P = 2p + sigma that keeps every rank's rows together."""
        return SlabPartition(2 * self.n, self.world, [2 * x for x in self.starts])

    def is_balanced(self):
        return self.starts == SlabPartition(self.n, self.world).starts
