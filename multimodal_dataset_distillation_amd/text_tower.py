"""TextTower: Python host of the frozen CLIP text tower (libmdd_hip.so `mdd_text_tower_*`; csrc/text_tower.hip).

What the reference's `textprocess` / `textprocess_train` (distill.py:107-144, networks.py:700-726) get from the `clip`
package for `--text_encoder clip`: `encode_text` of the published model -- token + positional embedding, pre-LN
QuickGELU blocks under a causal mask, `ln_final`, the row of the end-of-text token (the largest id of a sequence) times
`text_projection`.  Forward only; the weights are frozen and packed once at load.  Tokenising is not done here: the
tower takes the int token ids `clip.tokenize` produces.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import DTYPE_BF16, DTYPE_F32, MddTextTowerConfig, check

_DT = {"f32": DTYPE_F32, "fp32": DTYPE_F32, "float32": DTYPE_F32, "bf16": DTYPE_BF16, "bfloat16": DTYPE_BF16}
VARIANTS = ("clip_text_b32", "clip_text_micro", "clip_text_nano")
_IGNORED_PREFIXES = ("visual.", "model.visual.")
_IGNORED_NAMES = ("logit_scale", "model.logit_scale")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class TextTower:
    def __init__(self, variant="clip_text_b32", max_batch=2000, compute_dtype="bf16", device="cuda", bind=True):
        """max_batch: sequences per library call (`encode` splits longer inputs); compute_dtype: 'bf16' or 'f32' (storage
        and arithmetic of the blocks; the pooled row, ln_final and the projection are fp32 in both).  bind=False builds
        the tables only and needs no GPU."""
        if compute_dtype not in _DT:
            raise ValueError("compute_dtype must be 'bf16' or 'f32', got %r" % (compute_dtype,))
        self.lib = _lib.load()
        self.variant, self.max_batch, self.compute_dtype = variant, int(max_batch), compute_dtype
        self._variant_b = variant.encode()
        cfg = MddTextTowerConfig(self._variant_b, self.max_batch, _DT[compute_dtype])
        h = C.c_void_p()
        check(self.lib.mdd_text_tower_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.feature_dim = self.lib.mdd_text_tower_feature_dim(h)
        self.context = self.lib.mdd_text_tower_context(h)
        self.vocab = self.lib.mdd_text_tower_vocab(h)
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
        """[(name, shape, offset)] of the tower's flat fp32 parameter vector: the `clip` package's names under `model.`."""
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

    def load_state_dict_file(self, path):
        """A `torch.save`d name -> tensor mapping (e.g. `clip.load(...)[0].state_dict()`), read with weights_only=True."""
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

    def encode(self, ids):
        """ids [n, context] integers -> float32 [n, feature_dim] on the tower's device."""
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
