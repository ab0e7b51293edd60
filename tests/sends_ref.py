"""Bus sends restated in NumPy on top of downmix_ref (include/oalsfx_hip.h, "bus sends"): what the host's bookkeeping and the device
kernels are held to, bit for bit.

Every instance has SENDS sends, (bus, gain) each, and a send may carry a ramp (from, step, to, frames, done).  The members of a bus are
the (instance, send) pairs with that bus, by instance and inside an instance by send, in chunks of downmix_ref.CHUNK; a member's gain on
frame f of a call is e = from + float32(n) * step for n = done + f < frames -- product and sum rounded separately -- and `to` from there
on.  Every downmix advances every ramp by the call's frames."""
import numpy as np

import downmix_ref

SENDS = 4  # OALSFX_BUS_SENDS
MAX_RAMP = 1 << 24
f32 = np.float32


def ramp_gains(frm, step, to, frames, done, count, form="stated"):
    """e for n = done .. done + count - 1 as float32 [count].  form: "stated"; "running" (the reference's gain += step from `frm` on, what
    the contract is not); "fused" (from + n * step rounded once)."""
    n = np.arange(done, done + count, dtype=np.int64)
    with np.errstate(all="ignore"):
        if form == "stated":
            e = f32(frm) + n.astype(f32) * f32(step)
        elif form == "fused":
            e = (np.float64(f32(frm)) + n.astype(np.float64) * np.float64(f32(step))).astype(f32)
        else:
            run = np.empty(int(n[-1]) + 1 if count else 0, f32)
            g = f32(frm)
            for k in range(len(run)):
                run[k] = g
                g = f32(g + f32(step))
            e = run[done:]
    return np.where(n < frames, e, f32(to)).astype(f32)


class Sends:
    """The sends of a batch of n instances and the clock of their ramps."""

    def __init__(self, n):
        self.n = n
        self.bus = np.full((SENDS, n), -1, np.int64)
        self.bus[0] = 0
        self.gain = np.ones((SENDS, n), f32)
        self.frm = np.zeros((SENDS, n), f32)
        self.step = np.zeros((SENDS, n), f32)
        self.to = np.zeros((SENDS, n), f32)
        self.frames = np.zeros((SENDS, n), np.int64)  # 0: no ramp
        self.done = np.zeros((SENDS, n), np.int64)

    def now(self, send, i):
        """The gain the next frame gets."""
        if not self.frames[send, i]:
            return self.gain[send, i]
        return ramp_gains(self.frm[send, i], self.step[send, i], self.to[send, i], self.frames[send, i], self.done[send, i], 1)[0]

    def get(self, i, send=0):
        """(bus, gain, gain_to, frames_left), as oalsfx_batch_get_send_routing answers."""
        g = self.now(send, i)
        left = int(self.frames[send, i] - self.done[send, i])
        return int(self.bus[send, i]), g, (self.to[send, i] if left else g), left

    def set_routing(self, send, first, bus=None, gain=None):
        count = len(bus if bus is not None else gain)
        for k in range(count):
            if bus is not None:
                self.bus[send, first + k] = bus[k]
            if gain is not None:
                self.gain[send, first + k] = f32(gain[k])
                self.frames[send, first + k] = self.done[send, first + k] = 0

    def set_ramps(self, send, first, gain_to, frames):
        assert 0 <= frames <= MAX_RAMP
        for k, target in enumerate(gain_to):
            i = first + k
            start = self.now(send, i)
            self.frames[send, i] = self.done[send, i] = 0
            if frames == 0:
                self.gain[send, i] = f32(target)
                continue
            with np.errstate(all="ignore"):
                self.frm[send, i], self.to[send, i] = start, f32(target)
                self.step[send, i] = f32(f32(target) - start) / f32(frames)
            self.gain[send, i] = start
            self.frames[send, i] = frames

    def members(self, b):
        """[(instance, send)] of bus b in the stated order."""
        return [(i, s) for i in range(self.n) for s in range(SENDS) if self.bus[s, i] == b]

    def gains(self, i, s, count, form="stated"):
        if not self.frames[s, i]:
            return np.full(count, self.gain[s, i], f32)
        return ramp_gains(self.frm[s, i], self.step[s, i], self.to[s, i], self.frames[s, i], self.done[s, i], count, form)

    def advance(self, count):
        ramping = self.frames > 0
        self.done[ramping] = np.minimum(self.frames[ramping], self.done[ramping] + count)
        ended = ramping & (self.done == self.frames)
        self.gain[ended] = self.to[ended]
        self.frames[ended] = self.done[ended] = 0

    def downmix(self, x, n_buses, chunk=downmix_ref.CHUNK, form="stated", advance=True):
        """x: float32 [n][frames][channels].  Returns float32 [n_buses][frames][channels] and moves the clock on by the frames."""
        x = np.asarray(x, dtype=f32)
        assert x.shape[0] == self.n and self.bus.max() < n_buses
        out = np.zeros((n_buses,) + x.shape[1:], f32)
        with np.errstate(all="ignore"):
            for b in range(n_buses):
                members = self.members(b)
                acc = np.zeros(x.shape[1:], f32)
                for j in range(0, len(members), chunk):
                    p = np.zeros(x.shape[1:], f32)
                    for i, s in members[j:j + chunk]:
                        p = p + x[i] * self.gains(i, s, x.shape[1], form)[:, None]
                    acc = acc + p
                out[b] = acc
        if advance:
            self.advance(x.shape[1])
        return out


same_bits = downmix_ref.same_bits
