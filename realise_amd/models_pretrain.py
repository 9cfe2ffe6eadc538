"""Drop-in shell for the reference's ``Pho2Pretrain`` (src/models.py:1286-1347, driven by src/run_pretrain.py): the first stage of the
three-stage recipe (``pretrain_pho.sh`` -> ``pretrain_res.sh`` -> ``merge.py`` + fine-tuning).

The model is the pinyin branch of ``SpellBertPho2ResArch3`` alone - ``pho_embeddings`` -> ``pho_gru`` -> ``pho_model`` (4 layers) - under a
``BertOnlyMLMHead`` named ``cls2``, trained to predict every Chinese character of a sentence from its pinyin.  ``model_type`` 5 of the C
ABI: no bert stack, no fusion, no glyph tower, no output block; the engine's ``src_idx`` is the batch's ``tgt_idx`` (models.py:1319).

``forward(batch) -> (loss, pred_ids, active_labels)`` is the reference's tuple (models.py:1338-1347).  ``pred_ids`` /
``active_labels`` are ``[n_active]`` int64 in ascending row order, as the reference's boolean indexing gives them.  Neither is made from
``[B, S, V]`` logits: in training mode the cross-entropy row pass ranks the row it holds (``realise_engine_set_pred``), in evaluation
mode the decode epilogue of the classifier GEMM gives the top-1 id of every row and the active rows are gathered.  The returned tuple
is a ``PretrainOutput``: entry 0 (the loss) is there at once; entries 1 and 2 are cut to ``n_active`` when they are first read, which
is the one host read of the call - the reference pays the same read in ``prediction_scores[active_loss]``.  ``trainer.train`` reads
entry 0 only and stays free of host synchronisation.

``Pho2ResPretrain`` and ``ResPretrain`` (run_pretrain.py's 'pho2res-pretrain', models.py's glyph pretraining) are not implemented and are
refused by name (``config.variant_of``).

``merge_pretrained`` is merge.py:18-33: the hand-off of the pretrained encoders into the checkpoint fine-tuning starts from.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .modeling import RealiseModule, _EngineLoss, pinyin_table_for


class PretrainOutput(tuple):
    """``(loss, pred_ids, active_labels)``; the two id tensors are sliced to the active-row count on first access (one host read)."""

    def __new__(cls, loss, ids_buf, labels_buf, n_active, hits=None):
        self = super().__new__(cls, (loss,))
        self._loss, self._ids_buf, self._labels_buf, self._n_dev, self._hits_dev, self._cut = loss, ids_buf, labels_buf, n_active, hits, None
        return self

    def _materialise(self):
        if self._cut is None:
            n = int(self._n_dev.item())      # the host read
            self._cut = (self._ids_buf[:n], self._labels_buf[:n])
        return self._cut

    @property
    def hits(self):
        """0-d int32 device tensor: how many predictions equal their label (None from an evaluation forward: compare the ids)"""
        return self._hits_dev

    @property
    def n_active(self):
        """0-d int32 device tensor: the number of rows that entered the loss"""
        return self._n_dev

    def __len__(self):
        return 3

    def __getitem__(self, i):
        if isinstance(i, slice):
            return tuple(self[k] for k in range(*i.indices(3)))
        if i < 0:
            i += 3
        if i == 0:
            return self._loss
        if i in (1, 2):
            return self._materialise()[i - 1]
        raise IndexError(i)

    def __iter__(self):
        return iter((self[0], self[1], self[2]))


class Pho2Pretrain(RealiseModule):
    """src/models.py:1286-1347."""
    model_type = "pho2-pretrain"

    def __init__(self, config, compute_dtype=None, seed=0, init_scheme="reference", tie=False, logits_dtype=None):
        if tie:
            raise ValueError("Pho2Pretrain has no word table to tie cls2.predictions.decoder.weight to (models.py:1305): tie must be False")
        super().__init__(config, compute_dtype=compute_dtype, seed=seed, init_scheme=init_scheme, tie=False, logits_dtype=logits_dtype)
        self.train_logits = False    # forward returns ids, not logits: a bf16 training forward never allocates [B, S, V] (forward_logits does)
        self.last_logits = None      # [B, S, V] of the last forward that made logits (fp32 compute, or train_logits in bf16), else None

    def tie_cls_weight(self):
        raise RuntimeError("Pho2Pretrain has no word table to tie its decoder to")

    @staticmethod
    def build_batch(batch, tokenizer):
        """src/models.py:1309-1316: pinyin of the TARGET characters.  The vocabulary's table is built once per tokenizer and the batch is
        a gather; ``model.set_pinyin_table(pinyin_table_for(tokenizer))`` moves the gather to the device (``realise_build_pho``), and a
        batch without ``pho_idx`` is then completed there."""
        table = pinyin_table_for(tokenizer)
        tgt = batch["tgt_idx"]
        ids = tgt.detach().cpu().numpy() if torch.is_tensor(tgt) else np.asarray(tgt)
        pho_idx, pho_lens = table.convert(ids)
        batch["pho_idx"] = torch.from_numpy(np.ascontiguousarray(pho_idx))
        batch["pho_lens"] = pho_lens
        return batch

    def _no_token_tables(self):
        return "Pho2Pretrain reads the pinyin of tgt_idx, not of src_idx, and its evaluation is one short pass: there is no serving loop to table"

    def _engine_batch(self, batch):
        """the batch as the engine reads it: src_idx = tgt_idx (models.py:1319), so the range check, the device-side pinyin gather and the
        labels all see the same ids"""
        if "tgt_idx" not in batch or "loss_masks" not in batch:
            raise KeyError("Pho2Pretrain.forward needs tgt_idx, masks and loss_masks (models.py:1319-1321)")
        b = dict(batch)
        b["src_idx"] = batch["tgt_idx"]
        return b

    def _pred_buffers(self, n):
        cache = self.__dict__.setdefault("_pred_bufs", {})
        if n not in cache:
            i64 = dict(dtype=torch.int64, device=self.device)
            cache[n] = dict(ids=torch.empty(n, **i64), labels=torch.empty(n, **i64),
                            n=torch.zeros(1, dtype=torch.int32, device=self.device), hits=torch.zeros(1, dtype=torch.int32, device=self.device))
        return cache[n]

    def forward(self, batch):
        b = self._engine_batch(batch)
        self.last_logits = None
        if not self.training:
            return self._forward_eval(b)
        tgt = self._dev(b["tgt_idx"])
        n = tgt.numel()
        if n > 65536:
            raise ValueError("Pho2Pretrain ranks inside the cross-entropy pass over at most 65536 rows per batch, got %d" % n)
        bufs = self._pred_buffers(n)
        # fresh outputs per call: the caller may keep the tuple of an earlier step
        ids, labels = torch.empty_like(bufs["ids"]), torch.empty_like(bufs["labels"])
        n_act, hits = torch.zeros_like(bufs["n"]), torch.zeros_like(bufs["hits"])
        req = _capi.Pred()
        req.pred_ids, req.labels, req.n_active, req.hits, req.capacity = ids.data_ptr(), labels.data_ptr(), n_act.data_ptr(), hits.data_ptr(), n
        # installed for this one call (RealiseModule._install_requests, once the engine exists) and cleared behind it, whatever happens
        self._pred_req = req
        try:
            out = self._forward(b, 0)
        finally:
            self._pred_req = None
            if self._engine is not None:
                _capi.load().realise_engine_set_pred(self._engine, None)
        self.last_logits = out[1]
        self._last = (self._last or []) + [ids, labels, n_act, hits]
        return PretrainOutput(out[0], ids, labels, n_act[0], hits[0])

    _pred_req = None

    def _install_requests(self):
        if self._pred_req is not None:
            _capi.load().realise_engine_set_pred(self._engine, C.byref(self._pred_req))

    @torch.no_grad()
    def _forward_eval(self, b):
        """evaluation: the decode epilogue (k = 1), then the active rows gathered in ascending row order - no [B, S, V] tensor"""
        pred = self._forward(b, 1)
        tgt = self._dev(b["tgt_idx"]).reshape(-1)
        active = (self._dev(b["loss_masks"]).reshape(-1) == 1) & (tgt != -100)
        idx = active.nonzero().reshape(-1)       # (the host read: the boolean index of models.py:1343-1344)
        ids, labels = pred.ids.reshape(-1)[idx], tgt[idx]
        n = torch.tensor(idx.numel(), dtype=torch.int32, device=self.device)
        return PretrainOutput(pred.loss, ids, labels, n, (ids == labels).sum().to(torch.int32))

    def forward_logits(self, batch):
        """``(loss, logits [B, S, V])`` of the default forward - what ``RealiseModule.forward`` returns for the fine-tuning models; for
        callers and tests that want the scores themselves"""
        b = self._engine_batch(batch)
        keep = self.train_logits
        self.train_logits = True
        try:
            return self._forward(b, 0)
        finally:
            self.train_logits = keep

    @torch.no_grad()
    def predict(self, batch, topk=1):
        return super().predict(self._engine_batch(batch), topk)


def merge_pretrained(base_sd, pho_sd, res_sd=None):
    """merge.py:18-33 as a function of three state dicts: every key of ``pho_sd``, then of ``res_sd``, is copied onto ``base_sd`` (moved
    to the CPU, overwriting a key the base already has), then every key starting with ``position_embeddings.`` or ``char_images.``
    is dropped.  Returns the merged dict (a new dict; ``base_sd`` is not modified).  The result loads into the fine-tuning models with
    ``load_state_dict(strict=False)``: ``cls2.*`` of a Pho2Pretrain checkpoint is reported as unexpected, as in the reference."""
    out = dict(base_sd)
    for sd in (pho_sd, res_sd or {}):
        for k, v in sd.items():
            out[k] = v.to("cpu") if torch.is_tensor(v) else v
    for k in [k for k in out if k.startswith("position_embeddings.") or k.startswith("char_images.")]:
        del out[k]
    return out


MODEL_CLASSES = {          # src/run_pretrain.py:33-36 ('pho2res-pretrain' is not implemented: config.variant_of refuses it by name)
    "pho2-pretrain": Pho2Pretrain,
}
