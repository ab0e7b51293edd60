"""NumPy restatement of polyphony (include/oalsfx_hip.h, "polyphony"): every instance has K voices, each rendered by itself by
resample_ref.render_one, and the instance's input is (((+0.0f + o_0) + o_1) + ...) + o_(K-1): lanes ascending, every addition rounded
to float32 by itself.  Every voice's records advance by their own contracts."""
import numpy as np

import resample_ref as ref

f32 = np.float32
MAX_POLYPHONY = 16        # OALSFX_MAX_POLYPHONY


def mix(outs, leave_out=None):
    """outs [K][...] float32 -> the stated sum over the first axis.  leave_out [K][...] bool: terms that are not added at all (the
    contract allows it for a voice's frames that are +0.0f by the voice's own contract)."""
    acc = np.zeros(outs.shape[1:], f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(outs)):
            added = (acc + outs[k]).astype(f32)
            acc = added if leave_out is None else np.where(leave_out[k], acc, added)
    return acc


def render(records, envelopes, resamplers, tables, assets, frames, channels):
    """records [K][n] of sampler_ref.DTYPE, envelopes [K][n] of voice_ref.DTYPE, resamplers [K][n] (a table index or NONE), tables {index:
    coef [P][T]}, assets[k][i] the asset the voice (lane k, instance i) names.  Returns (out [n][frames][channels], the records
    afterwards [K][n], the envelopes afterwards [K][n])."""
    lanes, n = records.shape
    assert envelopes.shape == (lanes, n) and np.shape(resamplers) == (lanes, n) and 1 <= lanes <= MAX_POLYPHONY
    out = np.zeros((n, frames, channels), dtype=f32)
    after, env_after = records.copy(), envelopes.copy()
    for i in range(n):
        acc = np.zeros((frames, channels), f32)
        for k in range(lanes):
            coef = tables[int(resamplers[k][i])] if int(resamplers[k][i]) != ref.NONE else None
            o, after[k][i], env_after[k][i] = ref.render_one(records[k][i], envelopes[k][i], coef, assets[k][i], frames, channels)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = (acc + o).astype(f32)
        out[i] = acc
    return out, after, env_after
