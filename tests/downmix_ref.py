"""The bus downmix's arithmetic restated in NumPy (include/oalsfx_hip.h, "bus downmix"): what the device kernels are held to, bit for bit.

Per bus the members in ascending instance order, in chunks of CHUNK; per element a chunk's partial p = p + (x * gain) member after
member from +0.0f, then out = out + p chunk after chunk from +0.0f; fp32, product and sum rounded separately.  NumPy's float32 multiply
and add round once each and never fuse, and the loops below fix the order."""
import numpy as np

CHUNK = 32  # OALSFX_DOWNMIX_CHUNK


def downmix(x, bus, gain, n_buses, chunk=CHUNK):
    """x: float32 [n][frames][channels]; bus: n ints (-1: nowhere); gain: n float32.  Returns float32 [n_buses][frames][channels]."""
    x = np.asarray(x, dtype=np.float32)
    bus = np.asarray(bus)
    gain = np.asarray(gain, dtype=np.float32)
    out = np.zeros((n_buses,) + x.shape[1:], dtype=np.float32)
    with np.errstate(all="ignore"):
        for b in range(n_buses):
            members = np.nonzero(bus == b)[0]  # ascending
            acc = np.zeros(x.shape[1:], dtype=np.float32)
            for j in range(0, len(members), chunk):
                p = np.zeros(x.shape[1:], dtype=np.float32)
                for i in members[j:j + chunk]:
                    p = p + x[i] * gain[i]
                acc = acc + p
            out[b] = acc
    return out


def downmix_shards(x, bus, gain, n_buses, shards):
    """The group's arithmetic: `shards` is [(first, count)]; every shard sums its own instances (its chunks start at its first member),
    and the shards' buses are added in shard order from +0.0f."""
    out = np.zeros((n_buses,) + np.asarray(x).shape[1:], dtype=np.float32)
    with np.errstate(all="ignore"):
        for first, count in shards:
            out = out + downmix(x[first:first + count], np.asarray(bus)[first:first + count], np.asarray(gain)[first:first + count], n_buses)
    return out


def same_bits(got, want):
    """Bit patterns equal; where both are NaN the position is what counts (a NaN's sign and payload are not part of the contract)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(got) & np.isnan(want)
    return bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
