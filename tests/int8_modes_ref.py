"""Float64 decoding with the int8 options restated (DESIGN.md sections 37 and 38) over whole id rows: what
tests/test_mode_schedule_reference.py decodes its int8 neighbour pairs with and tests/test_gpu_int8_modes.py holds the
engine's full-length calls to.  The decoder is decoder_int8_ref.decoder_rows (quantized_weights for option decoder_int8),
the head logits_int8_ref's quantiser on the final LayerNorm rows and on the tied embedding (option logits_int8)."""
import numpy as np

import decoder_int8_ref as dref
from logits_int8_ref import F32, logits as logits_i8, quantize_rows


class Net:
    """A model file's decoder with either option on or off."""

    def __init__(self, dims, tensors):
        self.dims, self.tensors = dims, tensors
        self.E = np.asarray(tensors["decoder.token_embedding.weight"], np.float64)
        self.qweights = dref.quantized_weights(dims, tensors)
        self.qE = quantize_rows(np.asarray(tensors["decoder.token_embedding.weight"], F32))

    def ln_rows(self, row, enc, decoder_int8=False, cross_out=False):
        """final-LayerNorm rows [len(row)][d] in float64"""
        return dref.decoder_rows(self.dims, self.tensors, list(row), enc, self.qweights if decoder_int8 else None,
                                 cross_out=cross_out, want_logits=False)[1]

    def head(self, ln, logits_int8=False):
        """logits [rows][V] in float64 of final-LayerNorm rows"""
        ln = np.atleast_2d(ln)
        if not logits_int8:
            return ln @ self.E.T
        return logits_i8(*quantize_rows(ln.astype(F32)), *self.qE).astype(np.float64)

    def greedy(self, enc, prompt, max_pos, eot, decoder_int8=False, logits_int8=False, cross_out=False, stop_at_eot=True):
        """Greedy decoding over positions 0 .. max_pos - 1 (the last maximum wins a tie, as in the engine): (ids, the
        top-two margin of every choice)."""
        ids, margins = [int(i) for i in prompt], []
        while len(ids) <= max_pos:
            z = self.head(self.ln_rows(ids, enc, decoder_int8, cross_out)[-1], logits_int8)[0]
            tok = argmax_last(z)
            margins.append(float(z[tok] - np.delete(z, tok).max()))
            ids.append(tok)
            if stop_at_eot and tok == eot:
                break
        return ids, margins

    def forced(self, row, enc, n_prompt, decoder_int8=False, logits_int8=False, cross_out=False):
        """Teacher forcing on an id row: for every id behind the first n_prompt, its log-probability lp = z[id] -
        logsumexp(z) over the whole vocabulary (scores_ref's definition without timestamps), the last-maximum argmax of z
        and z's top-two margin; and the final-LayerNorm rows those logits came from."""
        row = [int(i) for i in row]
        ln = self.ln_rows(row[:-1], enc, decoder_int8, cross_out)[n_prompt - 1:]
        z = self.head(ln, logits_int8)
        m = z.max(axis=1)
        lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
        tok = np.asarray(row[n_prompt:])
        lp = z[np.arange(len(tok)), tok] - lse
        top = np.array([argmax_last(r) for r in z])
        second = np.partition(z, -2, axis=1)[:, -2]
        return dict(lp=lp, argmax=top, margin=m - second, ln=ln)


def argmax_last(x):
    x = np.asarray(x)
    return int(len(x) - 1 - np.argmax(x[::-1]))
