"""TextTower: Python host of the frozen text towers (libmdd_hip.so `mdd_text_tower_*`; csrc/text_tower.hip).

CLIP variants (`clip_text_*`)
-----------------------------

What the reference's `textprocess` / `textprocess_train` (distill.py:107-144, networks.py:700-726) get from the `clip`
package for `--text_encoder clip`: `encode_text` of the published model -- token + positional embedding, pre-LN
QuickGELU blocks under a causal mask, `ln_final`, the row of the end-of-text token (the largest id of a sequence) times
`text_projection`.  Forward only; the weights are frozen and packed once at load.  Tokenising is not done here: the
tower takes the int token ids `clip.tokenize` produces.

BERT variants (`bert_*`)
------------------------
What they get from `transformers` for `--text_encoder bert`, the reference's default (networks.py:703-735):
`BertModel("bert-base-uncased")(ids, attention_mask).last_hidden_state[:, 0]`, 768-d -- three embedding tables and an
embedding LayerNorm, post-LN blocks with exact GELU under a key-padding mask, the `[CLS]` row; no pooler.  The reference
pads a chunk to its longest caption and computes every padded row.  Here the tokens are PACKED: `encode` drops the padding
on the host, the linears run over sum(len) rows and the attention per sequence over its own keys
(csrc/attn_varlen.hip).  Tokenising is `transformers.BertTokenizer`'s job (embed_text.py calls it when the package is
there); the tower takes its `input_ids` and `attention_mask`.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import DTYPE_BF16, DTYPE_F32, MddTextTowerConfig, check

_DT = {"f32": DTYPE_F32, "fp32": DTYPE_F32, "float32": DTYPE_F32, "bf16": DTYPE_BF16, "bfloat16": DTYPE_BF16}
CLIP_VARIANTS = ("clip_text_b32", "clip_text_micro", "clip_text_nano")
BERT_VARIANTS = ("bert_base_uncased", "bert_micro", "bert_nano")
VARIANTS = CLIP_VARIANTS + BERT_VARIANTS
_IGNORED_PREFIXES = ("visual.", "model.visual.")
_IGNORED_NAMES = ("logit_scale", "model.logit_scale")
# BertModel / BertForPreTraining entries that are no part of the tower (after the optional `bert.` prefix is dropped)
_BERT_IGNORED_PREFIXES = ("pooler.", "cls.")
_BERT_IGNORED_NAMES = ("embeddings.position_ids", "embeddings.token_type_ids")
BERT_PAD_ID = 0         # [PAD] in BERT's vocabularies


def plan_calls(lens, max_batch, max_tokens):
    """[(first sequence, sequences, rows)] of the library calls that take sequences of the lengths `lens` in order: each
    call holds as many of the next sequences as fit in `max_batch` sequences and `max_tokens` rows.  ValueError when one
    sequence alone has more than `max_tokens` rows (or none at all)."""
    calls, first, cnt, rows = [], 0, 0, 0
    for i, n in enumerate(lens):
        n = int(n)
        if n < 1:
            raise ValueError("sequence %d is empty" % i)
        if n > max_tokens:
            raise ValueError("sequence %d has %d tokens, more than max_tokens = %d" % (i, n, max_tokens))
        if cnt == max_batch or rows + n > max_tokens:
            calls.append((first, cnt, rows))
            first, cnt, rows = i, 0, 0
        cnt, rows = cnt + 1, rows + n
    if cnt:
        calls.append((first, cnt, rows))
    return calls


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class TextTower:
    def __init__(self, variant="clip_text_b32", max_batch=2000, compute_dtype="bf16", device="cuda", bind=True,
                 max_tokens=0):
        """max_batch: sequences per library call (`encode` splits longer inputs); compute_dtype: 'bf16' or 'f32' (storage
        and arithmetic of the blocks; the pooled row, the last LayerNorm and CLIP's projection are fp32 in both).
        max_tokens (BERT variants): packed token rows per library call, which the workspace is planned from; 0 means
        max_batch * context, i.e. room for every sequence at full length.  bind=False builds the tables only and needs no
        GPU."""
        if compute_dtype not in _DT:
            raise ValueError("compute_dtype must be 'bf16' or 'f32', got %r" % (compute_dtype,))
        self.lib = _lib.load()
        self.variant, self.max_batch, self.compute_dtype = variant, int(max_batch), compute_dtype
        self._variant_b = variant.encode()
        self.is_bert = variant in BERT_VARIANTS
        if int(max_tokens) < 0:
            raise ValueError("max_tokens must not be negative, got %r" % (max_tokens,))
        cfg = MddTextTowerConfig(self._variant_b, self.max_batch, _DT[compute_dtype], int(max_tokens) if self.is_bert else 0)
        h = C.c_void_p()
        check(self.lib.mdd_text_tower_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.feature_dim = self.lib.mdd_text_tower_feature_dim(h)
        self.context = self.lib.mdd_text_tower_context(h)
        self.vocab = self.lib.mdd_text_tower_vocab(h)
        self.max_tokens = int(max_tokens) if self.is_bert and int(max_tokens) > 0 else self.max_batch * self.context
        self.param_numel = self.lib.mdd_text_tower_param_numel(h)
        self.workspace_bytes = self.lib.mdd_text_tower_workspace_bytes(h)
        self.workspace = self._ws_view = None
        self.loaded = False
        self.device = torch.device(device)
        if bind:
            self.bind()

    # ------------------------------------------------------------------ memory
    def bind(self):
        if not torch.cuda.is_available():
            raise RuntimeError("TextTower needs an MI355X (HIP device); there is no CPU path")
        try:
            self.workspace = torch.empty(self.workspace_bytes + 256, dtype=torch.uint8, device=self.device)
        except RuntimeError as e:
            raise RuntimeError("HIP out of memory allocating %.1f GiB text tower workspace: %s"
                               % (self.workspace_bytes / 2**30, e))
        off = (-self.workspace.data_ptr()) % 256
        self._ws_view = self.workspace[off:off + self.workspace_bytes]
        with torch.cuda.device(self.device):
            check(self.lib.mdd_text_tower_bind_workspace(self.h, C.c_void_p(self._ws_view.data_ptr()), self.workspace_bytes,
                                                         _stream()))
        self.loaded = False

    def close(self):
        if getattr(self, "h", None):
            self.lib.mdd_text_tower_destroy(self.h)
            self.h = None
        self.workspace = None
        self._ws_view = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def param_table(self):
        """[(name, shape, offset)] of the tower's flat fp32 parameter vector: the `clip` package's names under `model.`
        (CLIP), the bare `transformers` names of BertModel without `pooler.*` (BERT)."""
        out = []
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        ndim, off = C.c_int(), C.c_int64()
        for i in range(self.lib.mdd_text_tower_param_count(self.h)):
            check(self.lib.mdd_text_tower_param_info(self.h, i, name, 256, shape, C.byref(ndim), C.byref(off)))
            out.append((name.value.decode(), tuple(shape[:ndim.value]), off.value))
        return out

    def flat_from_state_dict(self, sd):
        """The flat fp32 CPU vector of a name -> tensor mapping, matched BY NAME.  Keys with or without the `model.`
        prefix, fp16 or fp32; `visual.*` and `logit_scale` are ignored.  ValueError when a name of the table is missing or
        has another shape."""
        if not isinstance(sd, dict):
            raise ValueError("expected a name -> tensor mapping, got %s" % type(sd).__name__)
        if self.is_bert:
            return self._bert_flat_from_state_dict(sd)
        by_name = {}
        for k, v in sd.items():
            k = str(k)
            if k.startswith(_IGNORED_PREFIXES) or k in _IGNORED_NAMES:
                continue
            by_name[k if k.startswith("model.") else "model." + k] = v
        flat = torch.empty(self.param_numel, dtype=torch.float32)
        for name, shape, off in self.param_table():
            if name not in by_name:
                raise ValueError("state dict lacks %r (with or without the 'model.' prefix)" % name[len("model."):])
            t = torch.as_tensor(by_name[name])
            if tuple(t.shape) != tuple(shape):
                raise ValueError("state dict entry %r has shape %s, the %s tower needs %s"
                                 % (name[len("model."):], tuple(t.shape), self.variant, tuple(shape)))
            n = int(np.prod(shape))
            flat[off:off + n] = t.detach().to(torch.float32).reshape(-1)
        return flat

    def _bert_flat_from_state_dict(self, sd):
        """BERT: keys bare or under `bert.` (BertForPreTraining and its kin), fp16 or fp32; `pooler.*`, `cls.*` and the
        `position_ids` / `token_type_ids` buffers are ignored."""
        by_name = {}
        for k, v in sd.items():
            k = str(k)
            if k.startswith("bert."):
                k = k[len("bert."):]
            if k.startswith(_BERT_IGNORED_PREFIXES) or k in _BERT_IGNORED_NAMES:
                continue
            by_name[k] = v
        flat = torch.empty(self.param_numel, dtype=torch.float32)
        for name, shape, off in self.param_table():
            if name not in by_name:
                raise ValueError("state dict lacks %r (with or without the 'bert.' prefix)" % name)
            t = torch.as_tensor(by_name[name])
            if tuple(t.shape) != tuple(shape):
                raise ValueError("state dict entry %r has shape %s, the %s tower needs %s"
                                 % (name, tuple(t.shape), self.variant, tuple(shape)))
            n = int(np.prod(shape))
            flat[off:off + n] = t.detach().to(torch.float32).reshape(-1)
        return flat

    def load_state_dict_file(self, path):
        """A `torch.save`d name -> tensor mapping (e.g. `clip.load(...)[0].state_dict()`, or
        `BertModel.from_pretrained(...).state_dict()`), read with weights_only=True."""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        self.load_flat(self.flat_from_state_dict(sd))

    def load_flat(self, theta):
        """theta: the flat fp32 vector of `param_table()` (any device).  Cast, packed and copied into the workspace once."""
        theta = torch.as_tensor(theta)
        if theta.dtype != torch.float32 or theta.numel() != self.param_numel:
            raise ValueError("theta must be float32 with %d elements, got %s with %d"
                             % (self.param_numel, theta.dtype, theta.numel()))
        if self._ws_view is None:
            raise RuntimeError("TextTower is not bound to a device (bind=False); there is no CPU path")
        th = theta.reshape(-1).to(self.device).contiguous()
        with torch.cuda.device(self.device):
            check(self.lib.mdd_text_tower_load(self.h, C.c_void_p(th.data_ptr()), _stream()))
            torch.cuda.current_stream().synchronize()      # theta may be freed once the copies have run
        self.loaded = True

    # ------------------------------------------------------------------ encode
    def check_ids(self, ids):
        """ids as an int32 CPU tensor [n, context]; ValueError for anything that is not an integer [n, context] array or
        holds an id outside [0, vocab) (the kernel would clamp it, silently embedding another token)."""
        t = torch.as_tensor(ids)
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError("token ids must be integers, got %s" % t.dtype)
        if t.dim() != 2 or t.shape[1] != self.context or t.shape[0] < 1:
            raise ValueError("token ids must be an [n, %d] array, got shape %s" % (self.context, tuple(t.shape)))
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= self.vocab:
            raise ValueError("token ids must lie in [0, %d), got values in [%d, %d]" % (self.vocab, lo, hi))
        return t.to(torch.int32)

    def pack(self, ids, attention_mask=None):
        """BERT: (packed int32 ids [sum(len)], lengths [n] as a list) of padded ids [n, L], L <= positions, on the CPU.
        attention_mask is what `batch_encode_plus(padding=True)` returns -- ones over a sequence, zeros over its padding;
        without one it is `ids != 0` ([PAD] is id 0 in BERT's vocabularies).  ValueError for a mask that is not ones
        followed by zeros in every row, an empty row, L > positions, or a valid id outside [0, vocab)."""
        t = torch.as_tensor(ids).cpu()
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError("token ids must be integers, got %s" % t.dtype)
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("token ids must be an [n, L] array, got shape %s" % (tuple(t.shape),))
        if t.shape[1] > self.context:
            raise ValueError("token ids are [n, %d]: longer than the %d positions of %s" % (t.shape[1], self.context, self.variant))
        if attention_mask is None:
            m = t != BERT_PAD_ID
        else:
            am = torch.as_tensor(attention_mask).cpu()
            if tuple(am.shape) != tuple(t.shape):
                raise ValueError("attention_mask has shape %s, the ids %s" % (tuple(am.shape), tuple(t.shape)))
            if am.dtype.is_floating_point or am.dtype.is_complex:
                raise ValueError("attention_mask must be integers or booleans, got %s" % am.dtype)
            if am.dtype != torch.bool and not bool(((am == 0) | (am == 1)).all()):
                raise ValueError("attention_mask must hold zeros and ones")
            m = am != 0
        if bool((m[:, 1:] & ~m[:, :-1]).any()):
            r = int((m[:, 1:] & ~m[:, :-1]).any(dim=1).nonzero()[0])
            raise ValueError("row %d: the mask is not ones followed by zeros (a padding position inside the sequence)" % r)
        lens = m.sum(dim=1)
        if int(lens.min()) < 1:
            raise ValueError("row %d is empty (no valid token)" % int((lens < 1).nonzero()[0]))
        packed = t[m]                                         # row-major: the sequences one after another
        lo, hi = int(packed.min()), int(packed.max())
        if lo < 0 or hi >= self.vocab:
            raise ValueError("token ids must lie in [0, %d), got values in [%d, %d]" % (self.vocab, lo, hi))
        return packed.to(torch.int32).contiguous(), lens.tolist()

    def _encode_bert(self, ids, attention_mask):
        packed, lens = self.pack(ids, attention_mask)
        calls = plan_calls(lens, self.max_batch, self.max_tokens)
        if self._ws_view is None:
            raise RuntimeError("TextTower is not bound to a device (bind=False); there is no CPU path")
        if not self.loaded:
            raise RuntimeError("TextTower has no weights: call load_state_dict_file or load_flat first")
        n = len(lens)
        # cu_seqlens of every call, one after another: call c's n_c + 1 entries start at first_c + c
        cu = []
        for first, cnt, _ in calls:
            cu += np.concatenate([[0], np.cumsum(lens[first:first + cnt])]).tolist()
        cu_d = torch.tensor(cu, dtype=torch.int32).to(self.device)
        ids_d = packed.to(self.device)
        out = torch.empty(n, self.feature_dim, dtype=torch.float32, device=self.device)
        row0 = 0
        with torch.cuda.device(self.device):
            for c, (first, cnt, rows) in enumerate(calls):
                check(self.lib.mdd_text_tower_encode_varlen(
                    self.h, C.c_void_p(ids_d[row0:].data_ptr()), C.c_void_p(cu_d[first + c:].data_ptr()), cnt, rows,
                    max(lens[first:first + cnt]), C.c_void_p(out[first:].data_ptr()), _stream()))
                row0 += rows
        return out

    def encode(self, ids, attention_mask=None):
        """CLIP: ids [n, context] integers -> float32 [n, feature_dim] on the tower's device.
        BERT: ids [n, L] (L <= positions) padded as `batch_encode_plus(padding=True)` pads, with its attention_mask (or
        none: `ids != 0`) -> float32 [n, width], the [CLS] rows of the last layer.  The padding is dropped on the host
        (`pack`) and the input is split, in order, into calls of at most max_batch sequences and max_tokens rows."""
        if self.is_bert:
            return self._encode_bert(ids, attention_mask)
        if attention_mask is not None:
            raise ValueError("a CLIP tower takes no attention_mask (its mask is causal)")
        ids = self.check_ids(ids)
        if self._ws_view is None:
            raise RuntimeError("TextTower is not bound to a device (bind=False); there is no CPU path")
        if not self.loaded:
            raise RuntimeError("TextTower has no weights: call load_state_dict_file or load_flat first")
        n = ids.shape[0]
        ids_d = ids.to(self.device).contiguous()
        out = torch.empty(n, self.feature_dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            for a in range(0, n, self.max_batch):
                b = min(n, a + self.max_batch)
                check(self.lib.mdd_text_tower_encode(self.h, C.c_void_p(ids_d[a:b].data_ptr()), b - a,
                                                     C.c_void_p(out[a:b].data_ptr()), _stream()))
        return out
