"""Textual inversion (Gal et al., 2022) on the HIP path: the denoiser and the text encoder stay frozen, and the only
trainable thing is the embedding vector of one or a few placeholder tokens.

    ti = mdm_hip.textual_inversion.attach(encoder, token_ids=[32100], init_ids=[1782])
    opt = torch.optim.AdamW(ti.parameters(), lr=5e-3)
    ...  trainer.train_batch(...)  /  loss.backward(); opt.step()

While attached, ``T5Encoder.forward`` reads the rows of ``ti.embeddings`` for the placeholder ids instead of the
vocabulary table (``mdm_t5_embed_rms_slots``); with grad mode on and ``embeddings.requires_grad`` it runs as one autograd
node whose backward is the chain of input gradients of csrc/text_encoder_bwd.hip.  No weight of the encoder gets a gradient.
Under ``no_grad`` (sampling) the override is honoured by the ordinary forward.  Graph capture of the differentiable
forward is not supported.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .text_encoder import T5Encoder


class TextualInversion(nn.Module):
    """The learned rows of an encoder: ``embeddings`` fp32 ``[P, D]``, row j standing for tokenizer id ``token_ids[j]``."""

    def __init__(self, encoder, token_ids, rows):
        super().__init__()
        self.__dict__["_encoder"] = encoder          # not a submodule: parameters() is the learned rows alone
        self.token_ids = [int(t) for t in token_ids]
        self.embeddings = nn.Parameter(rows.detach().clone().float().contiguous())
        self._tables = {}                            # device -> slot_of_id int32 [n_ids]

    @property
    def encoder(self):
        return self._encoder

    # ---- what the encoder reads --------------------------------------------------------------------------------------
    def _slot_of_id_host(self):
        vocab = self._encoder.config.vocab_size
        t = np.full(max(vocab, max(self.token_ids) + 1), -1, dtype=np.int32)
        t[self.token_ids] = np.arange(len(self.token_ids), dtype=np.int32)
        return t

    def _slot_table(self, device):
        device = torch.device(device)
        if device not in self._tables:
            self._tables[device] = torch.from_numpy(self._slot_of_id_host()).to(device)
        return self._tables[device]

    def _slot_index(self, plan, device):
        """inverted index of a packing plan for mdm_t5_embed_bwd: (slot_start int32 [P + 1], tokens int32 [n]), a slot's
        packed tokens ascending.  Host arithmetic when the ids came as a host array, a stable device sort otherwise."""
        P = len(self.token_ids)
        if plan["ids_h"] is not None:
            slots = self._slot_of_id_host()[plan["ids_h"]]
            order = np.argsort(slots, kind="stable")
            order = order[np.count_nonzero(slots < 0):]
            start = np.zeros(P + 1, dtype=np.int32)
            np.cumsum(np.bincount(slots[slots >= 0], minlength=P), out=start[1:])
            both = torch.from_numpy(np.concatenate([start, order.astype(np.int32)])).pin_memory().to(device, non_blocking=True)
            return both[:P + 1], both[P + 1:]
        table = self._slot_table(device)
        slots = table[plan["ids"].long().clamp(0, table.numel() - 1)]
        srt, order = torch.sort(slots, stable=True)
        start = torch.searchsorted(srt, torch.arange(P + 1, device=device, dtype=srt.dtype)).to(torch.int32)
        return start, order.to(torch.int32)

    # ---- state --------------------------------------------------------------------------------------------------------
    def get_extra_state(self):
        return {"token_ids": list(self.token_ids)}

    def set_extra_state(self, state):
        ids = [int(t) for t in state["token_ids"]]
        if len(ids) != len(self.token_ids):
            raise ValueError("state_dict holds %d placeholder tokens, this adapter %d" % (len(ids), len(self.token_ids)))
        _check_ids(ids)
        self.token_ids = ids
        self._tables.clear()

    # ---- lifecycle ----------------------------------------------------------------------------------------------------
    def detach(self):
        """the encoder is exactly as before ``attach`` (the learned rows stay in this object)"""
        enc = self._encoder
        if enc is not None and enc._adapter is self:
            enc.__dict__["_adapter"] = None
        return self

    @torch.no_grad()
    def merge(self):
        """write the learned rows into ``shared.weight`` and detach: the plain encoder then computes the same.  Only for
        ids inside the vocabulary -- an added token has no row to be written to."""
        enc = self._encoder
        vocab = enc.config.vocab_size
        beyond = [t for t in self.token_ids if t >= vocab]
        if beyond:
            raise _lib.MdmHipError("cannot merge placeholder ids %s: they lie beyond the vocabulary of %d rows (keep the "
                                   "adapter attached, or resize the table and re-attach)" % (beyond, vocab))
        w = enc.shared.weight
        w[torch.tensor(self.token_ids, device=w.device)] = self.embeddings.detach().to(w.device, w.dtype)
        return self.detach()


def _check_ids(ids):
    if not ids:
        raise ValueError("token_ids is empty")
    if min(ids) < 0:
        raise ValueError("negative token id in %s" % (ids,))
    if len(set(ids)) != len(ids):
        raise ValueError("duplicate token ids in %s" % (sorted(t for t in set(ids) if ids.count(t) > 1),))


def attach(encoder, token_ids, init_ids=None, init=None):
    """Make ``token_ids`` (tokenizer ids: inside the vocabulary -- a reused rare token -- or beyond ``vocab_size`` -- an
    added token) learnable on ``encoder``.  Initial rows: the table rows of ``init_ids`` (one per token), or ``init``
    ``[P, D]``, or by default the table rows of ``token_ids`` themselves where those exist."""
    if not isinstance(encoder, T5Encoder):
        raise TypeError("attach() takes an mdm_hip.T5Encoder, got %s" % type(encoder).__name__)
    if encoder._adapter is not None:
        raise _lib.MdmHipError("a textual inversion is already attached to this encoder: detach() it first")
    ids = [int(t) for t in (token_ids.tolist() if isinstance(token_ids, (torch.Tensor, np.ndarray)) else token_ids)]
    _check_ids(ids)
    table = encoder.shared.weight
    vocab, D, P = encoder.config.vocab_size, encoder.config.d_model, len(ids)
    if init is not None and init_ids is not None:
        raise ValueError("give init or init_ids, not both")
    if init is not None:
        init = torch.as_tensor(init)
        if tuple(init.shape) != (P, D):
            raise ValueError("init must be [%d, %d] (one row of d_model per token), got %s" % (P, D, tuple(init.shape)))
        rows = init.to(table.device)
    else:
        src = ids if init_ids is None else [int(t) for t in init_ids]
        if len(src) != P:
            raise ValueError("init_ids must name one table row per token: %d for %d tokens" % (len(src), P))
        bad = [t for t in src if not 0 <= t < vocab]
        if bad:
            raise ValueError("%s %s: no such row in the table of %d; pass init_ids or init for tokens beyond the vocabulary"
                             % ("token_ids" if init_ids is None else "init_ids", bad, vocab))
        rows = table.detach()[torch.tensor(src, device=table.device)]
    ti = TextualInversion(encoder, ids, rows)
    encoder.__dict__["_adapter"] = ti
    return ti
