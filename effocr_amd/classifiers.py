"""FFNN classifier recognizer on MI355X: the ``--N_classes`` mode of the reference.

``AutoClassifierFactory(backend, modelpath, n_classes)`` mirrors models/classifiers.py:35-83, where the recognizer is
``timm.create_model(name, num_classes=n_classes)`` and infer_effocr.py:329-333 turns its logits into ids with
``logits.argmax(-1)``.  Here the network is the package's encoder (``HipEncoder.forward(x, normalize=False)``, the embedding
before L2 normalisation, which is exactly the input of timm's head) followed by ``HipClassifierHead``: the head's
``nn.Linear`` in exact fp32 with the argmax fused behind it (libeffocr_head.so, include/effocr_head.h).

Only the ``"timm"`` backend and the architectures ``AutoEncoderFactory`` supports are implemented (the RegNets' head is ``head.fc``); ``"hf"``, XcitDinoClassifier
and anything else raise NotImplementedError, as the reference's ``else`` branch does.
"""
import ctypes

import torch

from . import _lib
from . import weights as W
from .encoders import DEFAULT_PRECISION, make_encoder


class HipClassifierHead:
    """Device-resident timm classifier head: fp32 weight [N, D] and bias [N] on one GPU.  ``__call__(emb)`` returns logits [B, N]
    float32, ``predict(emb)`` int64 ids [B] (torch.argmax(-1) semantics, no logits written); both are asynchronous on the current
    stream.  Every logit and id is bitwise independent of the call's batch size."""

    def __init__(self, weight, bias, device=None):
        self.device = _lib.require_gpu(device)
        self._L = _lib.head_lib()
        if weight.dim() != 2 or bias.dim() != 1 or bias.shape[0] != weight.shape[0]:
            raise ValueError(f"head weight [N,D] and bias [N] expected, got {tuple(weight.shape)} and {tuple(bias.shape)}")
        self.n_classes, self.in_features = int(weight.shape[0]), int(weight.shape[1])
        self.weight = weight.detach().to(self.device, torch.float32).contiguous()
        self.bias = bias.detach().to(self.device, torch.float32).contiguous()

    def _run(self, emb, want_logits, want_ids):
        if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.shape[1] != self.in_features:
            raise ValueError(f"expected embeddings [B,{self.in_features}], got {getattr(emb, 'shape', type(emb))}")
        if emb.dtype != torch.float32 or emb.device != self.device:
            raise ValueError(f"expected float32 embeddings on {self.device}, got {emb.dtype} on {emb.device}")
        emb = emb.contiguous()
        B = emb.shape[0]
        with torch.cuda.device(self.device):
            logits = torch.empty((B, self.n_classes), dtype=torch.float32, device=self.device) if want_logits else None
            ids = torch.empty((B,), dtype=torch.int64, device=self.device) if want_ids else None
            nbytes = int(self._L.effocr_classifier_head_workspace_bytes(B, self.n_classes)) if want_ids else 0
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device) if want_ids else None
            _lib.head_check(self._L.effocr_classifier_head(_lib.ptr(emb), B, self.in_features, _lib.ptr(self.weight),
                                                           _lib.ptr(self.bias), self.n_classes, _lib.ptr(logits), _lib.ptr(ids),
                                                           _lib.ptr(ws), ctypes.c_size_t(nbytes),
                                                           _lib.current_stream(self.device)), "effocr_classifier_head")
        return logits, ids

    def __call__(self, emb):
        return self._run(emb, True, False)[0]

    forward = __call__

    def predict(self, emb):
        return self._run(emb, False, True)[1]


def AutoClassifierFactory(backend, modelpath, n_classes, precision=DEFAULT_PRECISION, img_size=224, call_size_invariant=False):
    """Drop-in for models/classifiers.py:74 ``AutoClassifierFactory(backend, modelpath, n_classes)``: returns a class whose instances
    behave like the reference's ``AutoClassifier`` at its call sites — ``.load(ckpt)`` (``net.`` keys; infer_effocr.py:177),
    ``.to(device)`` / ``.eval()``, ``model(x[B,3,H,W]) -> logits [B, n_classes]`` float32 on the input's device (:330-332) — plus
    ``predict(x) -> ids [B]`` through the fused argmax.  ``precision`` / ``img_size`` / ``call_size_invariant`` are extensions with the
    encoders' defaults; the head itself always runs in fp32, bitwise independent of the call size."""
    if backend != "timm":
        raise NotImplementedError
    W.embed_dim(modelpath)          # raises NotImplementedError for unknown architectures
    n_classes = int(n_classes)
    if n_classes < 1:
        raise ValueError(f"n_classes must be >= 1, got {n_classes}")

    class AutoClassifier:
        arch = modelpath
        num_classes = n_classes

        def __init__(self, model=modelpath, device="cuda", seed=0):
            # the reference downloads ImageNet weights here (pretrained=True, classifiers.py:40); with no network the instance starts
            # from a seeded random init until load_state_dict()
            self.model_name = model
            self.img_size = img_size
            self._sd = W.init_state_dict(model, seed=seed, img_size=img_size, num_classes=n_classes)
            self._device = self._resolve(device)
            self._engine = None
            self._head = None
            self.training = False

        @staticmethod
        def _resolve(device):
            d = torch.device("cuda" if device is None else device)
            if d.type == "cuda" and d.index is None and torch.cuda.is_available():
                d = torch.device("cuda", torch.cuda.current_device())
            return d

        # -- checkpoint I/O (classifiers.py:56-60; train_effocr_recognizer.py:327 saves the timm model as `net.`) -----------------
        @classmethod
        def load(cls, checkpoint):
            ptnet = cls()
            ptnet.load_state_dict(W.load_checkpoint(checkpoint))
            return ptnet

        def load_state_dict(self, sd, strict=True):
            sd = W.strip_prefix(sd)
            W.check_state_dict(self.model_name, sd, img_size, num_classes=n_classes)
            self._sd = {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in sd.items()}
            self._engine = self._head = None

        def state_dict(self):
            return {"net." + k: v for k, v in self._sd.items()}

        # -- nn.Module look-alikes -----------------------------------------------------------------------------------------
        def to(self, device):
            device = self._resolve(device)
            if device != self._device:
                self._device, self._engine, self._head = device, None, None
            return self

        def eval(self):
            self.training = False
            return self

        def named_parameters(self):
            shapes = W.param_shapes(self.model_name, img_size, n_classes)
            for k, v in self._sd.items():
                if k in shapes and not k.endswith(("running_mean", "running_var")):
                    yield "net." + k, torch.nn.Parameter(v, requires_grad=True)

        def parameters(self):
            for _, p in self.named_parameters():
                yield p

        @property
        def engine(self):
            if self._engine is None:
                self._engine = make_encoder(self.model_name, self._sd, img_size=img_size, precision=precision, device=self._device,
                                            call_size_invariant=call_size_invariant)
            return self._engine

        @property
        def head(self):
            if self._head is None and W.is_levit(self.model_name):
                # two BatchNorm1d + Linear heads whose logits timm averages: folded on the host in float64 into one matrix
                w, b = W.levit_fold_heads(self._sd)
                self._head = HipClassifierHead(w, b, device=self._device)
            if self._head is None:
                wk, bk = W.head_keys(self.model_name)
                w = self._sd[wk]
                if w.dim() == 4:                         # BiT's head is a 1x1 convolution: [N, D, 1, 1] is the matrix [N, D]
                    w = w.reshape(w.shape[0], w.shape[1])
                self._head = HipClassifierHead(w, self._sd[bk], device=self._device)
            return self._head

        def embed(self, x):
            """The head's input: the encoder's embedding before L2 normalisation, [B, D] float32."""
            return self.engine.forward(x, normalize=False)

        def forward(self, x):
            return self.head(self.embed(x))

        def predict(self, x):
            """int64 ids [B] = forward(x).argmax(-1), through the fused argmax (no logits are written)."""
            return self.head.predict(self.embed(x))

        @property
        def call_size_invariant(self):
            """The engine's property of that name (HipEncoder.call_size_invariant); builds the engine."""
            return self.engine.call_size_invariant

        def check_status(self):
            """Raise if any forward since the last check produced a non-finite embedding (HipEncoder.check_status)."""
            if self._engine is not None:
                self._engine.check_status()

        __call__ = forward

    AutoClassifier.__name__ = "AutoClassifier"
    return AutoClassifier
