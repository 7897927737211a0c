"""Host side of the MI355X self-speculative decoding engine.

``HipEngine`` borrows a ``transformers.LlamaForCausalLM`` (the object the reference's strategies are
handed, reference self_speculation/generator_base.py:52-62), re-lays its projection weights once into
the MFMA-fragment layout the HIP kernels stream, owns the paged KV pool and the workspace, and exposes
the C-ABI entry points of ``include/layerskip_hip.h`` as methods.

PyTorch is used for storage and stream handles only: every tensor here is a buffer whose
``data_ptr()`` is passed to liblayerskip_hip.so.  No torch op computes anything on the decoding path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import LskConfig, LskStepResult

BUF_STEP = 0   # 16-row step buffer (draft rows / verify block)
BUF_BULK = 1   # prompt rows (prefill), doubles as the exit_query_cache of the first step
BUF_MSG = 2    # the layer pipeline's message: row 0 = header words, rows 1.. = the verify block (lsk_pipeline_*)


@dataclass
class StepResult:
    """What ``single_step_speculation`` returns in the reference (SSG:223-229) plus the tokens."""
    num_matches: int
    num_drafts: int
    next_token: int
    kv_len: int
    emitted: List[int]
    draft_tokens: List[int]
    verified_tokens: List[int]


@dataclass
class ScoreResult:
    """What ``HipEngine.score`` returns: position i of row k is the model's prediction for ``ids[i + 1]`` after layers
    ``[0, layer_ends[k])`` (final norm + lm_head on that hidden state)."""
    ids: List[int]
    layer_ends: List[int]
    logprobs: torch.Tensor      # fp32 [E, n - 1]: log-probability of ids[1:]
    argmax: torch.Tensor        # int32 [E, n - 1]: the greedy token at each position

    @property
    def greedy(self) -> torch.Tensor:
        """bool [E, n - 1]: the greedy token is the next id (eval.py:301-305's `max_equal`, per position)."""
        return self.argmax == torch.tensor(self.ids[1:], dtype=torch.int32)

    def nll(self, k: int = -1) -> float:
        """Mean negative log-likelihood per token at ``layer_ends[k]`` (perplexity = exp of it)."""
        return float(-self.logprobs[k].double().mean())


def _round_up(v: int, a: int) -> int:
    return (v + a - 1) // a * a


def _i32_array(values: Sequence[int]):
    arr = (ctypes.c_int32 * max(1, len(values)))()
    for i, v in enumerate(values):
        arr[i] = int(v)
    return arr


def _u64(v: int) -> int:
    """A Philox key / counter as the uint64_t the C ABI takes."""
    return int(v) & (2 ** 64 - 1)


def _host_ids(input_ids: Optional[Sequence[int]]):
    """(ids array, count) of optional host ids: None = a block that continues on the device (NULL, 1)."""
    if input_ids is None:
        return None, 1
    return _i32_array(input_ids), len(input_ids)


class HipEngine:
    """One engine per (model, device).  Not re-entrant; one caller thread (like the reference)."""

    def _ck(self, status: int) -> None:
        _lib.check(status, self.lib)

    def _eos_array(self, eos_token_ids: Sequence[int]):
        """The eos list as the device sees it: ids outside the vocabulary can never be produced and are dropped, repeats are dropped
        (first occurrence kept: the list ORDER decides which id truncates the output, SSG:82-91).  The reference folds any number of
        `stop_token_ids` into this list (generator_base.py:106); the device list holds LSK_MAX_EOS = 1024 -- more than that is an error,
        never a silent truncation (the device-side draft cut and the host-side output cut must agree)."""
        eos = list(dict.fromkeys(int(t) for t in eos_token_ids if t is not None and 0 <= int(t) < self.vocab))     # None: a tokenizer without eos
        if len(eos) > _lib.LSK_MAX_EOS:
            raise _lib.LskError(f"{len(eos)} distinct eos / stop token ids; the engine supports at most {_lib.LSK_MAX_EOS}")
        return eos, _i32_array(eos)

    def __init__(self, model, max_ctx: int = 2048, max_prompt: int = 1024, page_size: int = 128,
                 target_wgs: int = 0, layer_range: Optional[Sequence[int]] = None, release_weights: bool = False,
                 weight_format: str = "bf16", draft_weight_format: Optional[str] = None, draft_layers: Optional[int] = None):
        cfg = model.config
        if weight_format not in _lib.WEIGHT_FORMATS:
            raise _lib.LskError(f"unknown weight_format {weight_format!r} ({' | '.join(_lib.WEIGHT_FORMATS)})")
        if draft_weight_format is not None:
            if draft_weight_format not in ("fp8_e4m3", "mxfp4"):
                raise _lib.LskError(f"unknown draft_weight_format {draft_weight_format!r} (fp8_e4m3 | mxfp4)")
            if weight_format != "bf16":
                raise _lib.LskError(f"draft_weight_format={draft_weight_format!r} needs weight_format='bf16', not {weight_format!r}: "
                                    "the copies are for drafting, what is kept comes from the bf16 weights")
            if layer_range is not None:
                raise _lib.LskError("draft_weight_format is a one-GPU option: a layer-range engine (pipeline rank) takes no draft copies")
            if draft_layers is not None and not (1 <= int(draft_layers) <= cfg.num_hidden_layers):
                raise _lib.LskError(f"draft_layers={draft_layers} out of range 1..{cfg.num_hidden_layers}")
        elif draft_layers is not None:
            raise _lib.LskError("draft_layers needs a draft_weight_format")
        # (the final norm is the one tensor every rank of a pipeline materialises: a middle rank holds neither the embedding nor the head)
        weight = model.model.norm.weight if model.model.embed_tokens.weight.is_meta else model.model.embed_tokens.weight
        dmap = getattr(model, "hf_device_map", None)
        if dmap and len(set(dmap.values())) > 1:
            # the reference's multi-GPU form (generate.py:59-64): ONE process, layers spread by accelerate hooks
            raise _lib.LskError("this model was spread over several devices by device_map='auto'; the engine wants one process per GPU: "
                                "launch the driver under torchrun (every rank loads its own layer range, layerskip_amd/checkpoint.py) "
                                "or load the model on one device")
        if weight.device.type != "cuda":
            raise _lib.LskError("HipEngine needs the model on a HIP device (model.to('cuda')); there is no CPU path")
        if weight.dtype == torch.bfloat16:
            self.dtype, dtype_name = torch.bfloat16, "bf16"
        elif weight.dtype == torch.float16:
            # the fp16 library: the same sources built with -DLSK_ELEM_F16 (the dtype generate.py:63 hard-codes)
            self.dtype, dtype_name = torch.float16, "fp16"
        elif weight.dtype == torch.float32:
            # the fp32 library: -DLSK_ELEM_F32 (HF's default dtype, the one the reference's unit tests load)
            self.dtype, dtype_name = torch.float32, "fp32"
        else:
            raise _lib.LskError(f"HipEngine computes in bf16, fp16 or fp32; model dtype is {weight.dtype}")
        # weight_format="fp8_e4m3" (opt-in; "bf16" = the model dtype, the default): the projections are stored as e4m3 codes with one
        # power of two per output row (layerskip_amd/quant.py) and the decode path streams half the bytes; bit-identical to this engine
        # in bf16 on quant.dequantized_model(model).  The bf16 library only.
        # weight_format="mxfp4" (opt-in): q/k/v/o/gate/up/down as OCP MXFP4 (e2m1 codes, one power of two per 32-feature block), the
        # lm_head in the FP8 format; bit-identical to this engine in bf16 on quant.dequantized_model(model, "mxfp4").
        if weight_format != "bf16" and dtype_name != "bf16":
            raise _lib.LskError(f"weight_format={weight_format!r} needs a bf16 model; this one is {dtype_name} "
                                "(FP8 weight storage exists in the bf16 build only)")
        self.weight_format = weight_format
        # draft_weight_format="fp8_e4m3" | "mxfp4" (opt-in; None = off): quantised COPIES of the projections of layers [0, draft_layers)
        # (default: every layer) and an FP8 copy of the lm_head, read by the one-row draft passes of a speculation step only.  The
        # verify block then runs all layers from the bf16 weights and rewrites the early layers' KV, so KV, verified logits and emitted
        # tokens are the plain engine's bit for bit -- on any checkpoint; only acceptance moves.
        if draft_weight_format is not None and dtype_name != "bf16":
            raise _lib.LskError(f"draft_weight_format={draft_weight_format!r} needs a bf16 model; this one is {dtype_name} "
                                "(quantised draft copies exist in the bf16 build only)")
        self.draft_weight_format = draft_weight_format
        self.draft_layers = (cfg.num_hidden_layers if draft_layers is None else int(draft_layers)) if draft_weight_format is not None else 0
        # what the MFMA-tiled prefill kernels read under FP8: the same codes as the decode kernels (their FP8 instances widen them in
        # the weight ring and scale the accumulators, csrc/lsk_gemm_big.h), so prompt KV and exit hiddens are the bf16 engine's on the
        # dequantised model and packed bytes are 0.5 x bf16's.  None in the default format.  One set of buffers serves both paths.
        # Under MXFP4 no prefill kernel reads the codes: the engine widens one layer at a time into a layer-sized bf16 scratch
        # (_allocate) and the model-dtype prefill kernels read that.
        self.prefill_weights = {"fp8_e4m3": "fp8_codes", "mxfp4": "mxfp4_layer_scratch"}.get(weight_format)
        self.lib = _lib.load(dtype=dtype_name)
        self.elem_bytes = torch.empty(0, dtype=self.dtype).element_size()
        # sample=True on the device: the sampler's 16-bit logit keys are exact at bf16 / fp16 only (lsk_key16, lsk_sample.h).  Over fp32
        # logits they would merge distinct values and top-k / top-p would act on other sets than the reference's warpers, so the fp32
        # engine offers no device-sampled entry point: the strategies read this flag and keep sampled steps on the host path.
        self.samples_on_device = self.lib.lsk_elem_dtype() != _lib.DTYPE_CODES["fp32"]
        if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False):
            raise _lib.LskError("biased projections are not supported")
        # The engine keeps its own references to every tensor it borrows (embedding, norm gains) and copies of the
        # scalars it needs later, but NOT the model: `get_engine` maps model -> engine weakly, and a strong
        # reference back to the key would keep both (and ~2x the weights in HBM) alive forever.
        import weakref
        self._model_ref = weakref.ref(model)
        self.rms_eps = float(cfg.rms_norm_eps)
        rot = model.model.rotary_emb
        self._inv_freq = rot.inv_freq.detach().to("cpu", torch.float32).clone()
        self._rope_scaling = float(rot.attention_scaling)
        self.device = weight.device
        self.num_layers = cfg.num_hidden_layers
        self.hidden = cfg.hidden_size
        self.intermediate = cfg.intermediate_size
        self.n_heads = cfg.num_attention_heads
        self.n_kv_heads = cfg.num_key_value_heads
        self.head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        self.vocab = cfg.vocab_size
        self.page_size = page_size
        self.target_wgs = target_wgs
        self.layer_range = tuple(layer_range) if layer_range is not None else (0, self.num_layers)
        # release_weights: after a projection is packed its HF original is dropped (the model object then
        # only serves this engine) -- what lets a 70B checkpoint (140 GB bf16) live on ONE 288 GB MI355X
        self.release_weights = release_weights
        self._handle = ctypes.c_void_p(None)
        self._packed = []           # per-layer packed buffers (kept alive); None outside layer_range
        self._packed_draft = []     # draft_weight_format: (wqkv, wo, wgu, wdown) copies of layers [0, draft_layers)
        self._packed_prefill = {}   # measurement only (_bind_prefill_copies): layer -> bf16-packed dequantised copies for the prefill kernels
        self._globals = {}
        self._buffers = {}
        self._options = {}          # lsk_engine_set_option values, re-applied whenever the C engine is recreated
        self._block_table = None
        self._profile = False
        self._fingerprint = None
        with torch.cuda.device(self.device):
            self._pack_weights(model)
            self._allocate(max_ctx, max_prompt)
        self._fingerprint = self._weights_fingerprint(model)

    @property
    def model(self):
        """The borrowed model, or None once the caller dropped it (the engine keeps working: it owns packed
        copies of the projections and references to the tensors it shares)."""
        return self._model_ref()

    # ------------------------------------------------------------------ weights
    def _weight_tensors(self, m):
        out = []
        for idx, layer in enumerate(m.model.layers):
            if not (self.layer_range[0] <= idx < self.layer_range[1]):
                continue
            a, mlp = layer.self_attn, layer.mlp
            out += [a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.o_proj.weight, mlp.gate_proj.weight, mlp.up_proj.weight,
                    mlp.down_proj.weight, layer.input_layernorm.weight, layer.post_attention_layernorm.weight]
        out += [t for t in (m.lm_head.weight, m.model.embed_tokens.weight, m.model.norm.weight) if not t.is_meta]
        return out

    def _weights_fingerprint(self, m):
        """What the engine copied or borrowed, in two parts: (storage address, in-place version) of every tensor --
        load_state_dict(), an in-place op on the Parameter or assigning a new Parameter shows there -- and a sampled CONTENT
        checksum per tensor (lsk_engine_weights_checksum: up to 4096 evenly strided elements each, one launch), because an
        edit through `.data` (`p.data += delta`: PEFT's default LoRA merge) moves neither the address nor the version.  An edit
        confined to elements the sample misses is not detected: call refresh_weights() after such surgery."""
        if self.release_weights:
            return None                      # the originals were dropped: the model object only serves this engine
        tensors = self._weight_tensors(m)
        meta = tuple((t.data_ptr(), t._version) for t in tensors)
        if not self._handle or any(t.device != self.device or t.element_size() != self.elem_bytes or not t.is_contiguous() for t in tensors):
            return (meta, None)
        n = len(tensors)
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
        cnts = (ctypes.c_int64 * n)(*[t.numel() * self.elem_bytes // 2 for t in tensors])    # the checksum samples 2-byte units
        sums = (ctypes.c_uint64 * n)()
        self._ck(self.lib.lsk_engine_weights_checksum(self._handle, ptrs, cnts, n, sums, self._stream))
        return (meta, tuple(sums))

    def weights_changed(self, model=None) -> bool:
        model = model if model is not None else self.model
        if model is None or self._fingerprint is None:
            return False
        return self._weights_fingerprint(model) != self._fingerprint

    def refresh_weights(self, model=None) -> None:
        """Re-pack every projection from the model's CURRENT weights and re-bind the borrowed tensors (after
        load_state_dict / in-place edits / a LoRA merge on the same model object).  The cached context is dropped."""
        model = model if model is not None else self.model
        if model is None:
            raise _lib.LskError("refresh_weights: the model this engine was built from is gone")
        if self.release_weights:
            raise _lib.LskError("refresh_weights: this engine released the original weights (release_weights=True)")
        with torch.cuda.device(self.device):
            self._bind_prefill_copies(list(self._packed_prefill), bind=False)      # (copies of the old values, if a tool bound any)
            self._packed = []
            self._packed_draft = []
            self._globals = {}
            self._pack_weights(model)
            self._bind_weights()
        self._fingerprint = self._weights_fingerprint(model)
        self.reset()

    @property
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def _fp8(self) -> bool:
        return self.weight_format == "fp8_e4m3"

    @property
    def _head_format(self) -> str:
        """The format of the packed lm_head: the engine's, except that an MXFP4 engine keeps its head in the FP8 format."""
        return "fp8_e4m3" if self.weight_format == "mxfp4" else self.weight_format

    def _packed_buffer(self, n_rows: int, k: int, fmt: str):
        """The packed buffer of an [n_rows][k] projection in format `fmt` (FP8: the codes, then one fp32 power of two per packed row;
        MXFP4: the codes, then the blocks' exponent bytes)."""
        nbytes = ctypes.c_size_t(0)
        fn = {"bf16": self.lib.lsk_packed_bytes, "fp8_e4m3": self.lib.lsk_packed_bytes_fp8, "mxfp4": self.lib.lsk_packed_bytes_mxfp4}[fmt]
        self._ck(fn(n_rows, k, ctypes.byref(nbytes)))
        return torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)

    def _pack_into(self, dst, w: torch.Tensor, tile_offset: int, tile_stride: int, rope_hd: int, fmt: str, dst_rows: int = 0) -> None:
        """`dst_rows`: the rows of the whole destination (a multiple of 16), which locate the scale table of the quantised formats."""
        w = w.detach()
        if w.dtype != self.dtype or w.device != self.device:
            raise _lib.LskError(f"all projection weights must be {self.dtype} on the engine's device")
        if w.stride(1) != 1:
            w = w.contiguous()
        if fmt == "bf16":
            self._ck(self.lib.lsk_pack_linear(w.data_ptr(), w.shape[0], w.shape[1], w.stride(0), dst.data_ptr(),
                                           tile_offset, tile_stride, rope_hd, self._stream))
            return
        fn = self.lib.lsk_pack_linear_fp8 if fmt == "fp8_e4m3" else self.lib.lsk_pack_linear_mxfp4
        self._ck(fn(w.data_ptr(), w.shape[0], w.shape[1], w.stride(0), dst.data_ptr(), dst_rows, tile_offset, tile_stride, rope_hd,
                    self._stream))

    def _pack_projections(self, layer, fmt: str, values=lambda w: w):
        """(wqkv, wo, wgu, wdown) of one decoder layer, packed in format `fmt`: q|k|v concatenated (q and k in RoPE row order), gate / up
        interleaved by tile.  `values` maps a weight to what is packed in its place.  Nothing here synchronises."""
        hd, H, I = self.head_dim, self.hidden, self.intermediate
        qdim, kvdim = self.n_heads * hd, self.n_kv_heads * hd
        a, mlp = layer.self_attn, layer.mlp
        plan = ((qdim + 2 * kvdim, H, ((a.q_proj, 0, 1, hd), (a.k_proj, qdim // 16, 1, hd), (a.v_proj, (qdim + kvdim) // 16, 1, 0))),
                (H, qdim, ((a.o_proj, 0, 1, 0),)),
                (2 * I, H, ((mlp.gate_proj, 0, 2, 0), (mlp.up_proj, 1, 2, 0))),
                (H, I, ((mlp.down_proj, 0, 1, 0),)))
        out = []
        for n_rows, k, parts in plan:
            buf = self._packed_buffer(n_rows, k, fmt)
            for lin, tile_offset, tile_stride, rope_hd in parts:
                self._pack_into(buf, values(lin.weight), tile_offset, tile_stride, rope_hd, fmt, _round_up(n_rows, 16))
            out.append(buf)
        return tuple(out)

    def packed_weight_bytes(self) -> dict:
        """Bytes of the packed projection buffers (this engine's layers and its lm_head): "decode" -- the buffers the decode path reads,
        which in the bf16 and FP8 formats are the ones prefill reads too; "prefill_only" -- buffers that only the prefill kernels read
        (0); on an MXFP4 engine only, "prefill_scratch" -- the layer-sized bf16 scratch it widens one layer at a time into; and, with
        draft_weight_format only, "draft" -- the quantised copies the draft passes read and the FP8 draft head."""
        bufs = [t for pk in self._packed if pk is not None for t in pk[:4]]
        bufs += [self._globals["lm_head"]] if self._globals.get("lm_head") is not None else []
        out = {"decode": sum(t.numel() for t in bufs),
               "prefill_only": sum(t.numel() for pk in self._packed_prefill.values() for t in pk)}
        if self.draft_weight_format is not None:         # the draft copies and the FP8 draft head
            out["draft"] = sum(t.numel() for pk in self._packed_draft for t in pk) + self._globals["draft_head"].numel()
        if self._buffers.get("prefill_scratch") is not None:
            out["prefill_scratch"] = self._buffers["prefill_scratch"].numel()
        return out

    def _bind_prefill_copies(self, layers=None, bind: bool = True) -> None:
        """A/B lever of tools/ and tests/, FP8 and MXFP4 engines only: bf16-packed copies of the DEQUANTISED projections of `layers` (default: all of
        this engine's), bound with lsk_engine_set_layer_prefill, so that those layers prefill through the model-dtype kernels -- what
        every FP8 engine did before the prefill kernel read the codes.  bind=False unbinds and frees them."""
        from . import quant
        for i in (range(*self.layer_range) if layers is None else layers):
            if bind:
                self._packed_prefill[i] = self._pack_projections(self.model.model.layers[i], "bf16",
                                                                 lambda w: quant.dequantize_weight(w, self.weight_format))
                torch.cuda.synchronize(self.device)          # the dequantised values are temporaries: the pack kernels must be through
                ptrs = [t.data_ptr() for t in self._packed_prefill[i]]
            else:
                ptrs = [None] * 4
                self._packed_prefill.pop(i, None)
            self._ck(self.lib.lsk_engine_set_layer_prefill(self._handle, i, *ptrs))

    def unpacked_fp8(self, layer: int, name: str):
        """(codes uint8 [rows][k], scale fp32 [rows]) of a packed FP8 buffer in PACKED row order (quant.unpack_tiles); name: wqkv | wo |
        wgu | wdown | lm_head."""
        if not (self._fp8 or (self.weight_format == "mxfp4" and name == "lm_head")):
            raise _lib.LskError("unpacked_fp8: this buffer of the engine is not stored as FP8")
        from . import quant
        hd, H, I = self.head_dim, self.hidden, self.intermediate
        shapes = {"wqkv": ((self.n_heads + 2 * self.n_kv_heads) * hd, H), "wo": (H, self.n_heads * hd), "wgu": (2 * I, H),
                  "wdown": (H, I), "lm_head": (self.vocab, H)}
        buf = self._globals["lm_head"] if name == "lm_head" else self._packed[layer][("wqkv", "wo", "wgu", "wdown").index(name)]
        return quant.unpack_tiles(buf, *shapes[name])

    def unpacked_mxfp4(self, layer: int, name: str):
        """(codes uint8 [rows][k/2], exp uint8 [rows][k/32]) of a packed MXFP4 buffer in PACKED row order (quant.unpack_tiles_mxfp4);
        name: wqkv | wo | wgu | wdown (the lm_head of an MXFP4 engine is FP8: unpacked_fp8)."""
        if self.weight_format != "mxfp4":
            raise _lib.LskError("unpacked_mxfp4: this engine does not store its weights as MXFP4")
        from . import quant
        hd, H, I = self.head_dim, self.hidden, self.intermediate
        shapes = {"wqkv": ((self.n_heads + 2 * self.n_kv_heads) * hd, H), "wo": (H, self.n_heads * hd), "wgu": (2 * I, H), "wdown": (H, I)}
        return quant.unpack_tiles_mxfp4(self._packed[layer][("wqkv", "wo", "wgu", "wdown").index(name)], *shapes[name])

    def _pack_weights(self, m) -> None:
        H = self.hidden
        for idx, layer in enumerate(m.model.layers):
            if not (self.layer_range[0] <= idx < self.layer_range[1]):
                self._packed.append(None)       # another pipeline rank owns this layer
                continue
            a, mlp = layer.self_attn, layer.mlp
            n1 = layer.input_layernorm.weight.detach().contiguous()
            n2 = layer.post_attention_layernorm.weight.detach().contiguous()
            self._packed.append(self._pack_projections(layer, self.weight_format) + (n1, n2))
            if idx < self.draft_layers:
                self._packed_draft.append(self._pack_projections(layer, self.draft_weight_format))
            if self.release_weights:
                torch.cuda.synchronize(self.device)
                for lin in (a.q_proj, a.k_proj, a.v_proj, a.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj):
                    lin.weight = torch.nn.Parameter(torch.empty(0, dtype=self.dtype, device=self.device),
                                                    requires_grad=False)
        # a pipeline rank that runs no head / embeds no token (checkpoint.load_layer_range(embed=False, head=False)) leaves them on meta
        have_head, have_embed = not m.lm_head.weight.is_meta, not m.model.embed_tokens.weight.is_meta
        self._globals["lm_head"] = None
        if have_head:
            head = self._packed_buffer(self.vocab, H, self._head_format)
            self._pack_into(head, m.lm_head.weight, 0, 1, 0, self._head_format, _round_up(self.vocab, 16))
            self._globals["lm_head"] = head
            if self.draft_weight_format is not None:
                dhead = self._packed_buffer(self.vocab, H, "fp8_e4m3")
                self._pack_into(dhead, m.lm_head.weight, 0, 1, 0, "fp8_e4m3", _round_up(self.vocab, 16))
                self._globals["draft_head"] = dhead
            tied = have_embed and m.lm_head.weight.data_ptr() == m.model.embed_tokens.weight.data_ptr()
            if self.release_weights and not tied:
                torch.cuda.synchronize(self.device)
                m.lm_head.weight = torch.nn.Parameter(torch.empty(0, dtype=self.dtype, device=self.device),
                                                      requires_grad=False)
        self._globals["embed"] = m.model.embed_tokens.weight.detach().contiguous() if have_embed else None
        self._globals["final_norm"] = m.model.norm.weight.detach().contiguous() if have_head else None
        torch.cuda.synchronize(self.device)

    def _rope_tables(self, length: int):
        """cos/sin exactly as LlamaRotaryEmbedding.forward computes them on CPU (fp32 -> model dtype)."""
        inv_freq, scaling = self._inv_freq, self._rope_scaling
        pos = torch.arange(length, dtype=torch.float32)
        freqs = (inv_freq[None, :, None] @ pos[None, None, :]).transpose(1, 2)[0]   # [length, d/2]
        cos = (freqs.cos() * scaling).to(self.dtype)
        sin = (freqs.sin() * scaling).to(self.dtype)
        return cos.contiguous().to(self.device), sin.contiguous().to(self.device)

    # ------------------------------------------------------------------ buffers / C engine
    def _allocate(self, max_ctx: int, max_prompt: int) -> None:
        if self._handle:
            self._ck(self.lib.lsk_engine_destroy(self._handle))
            self._handle = ctypes.c_void_p(None)
        self.max_ctx = _round_up(max(max_ctx, self.page_size), self.page_size)
        self.max_prompt = max(16, int(max_prompt))
        self.cfg = LskConfig(self.num_layers, self.hidden, self.intermediate, self.n_heads, self.n_kv_heads,
                             self.head_dim, self.vocab, self.rms_eps, self.max_ctx, self.page_size,
                             self.max_prompt, self.target_wgs)
        ws, kv = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._ck(self.lib.lsk_workspace_bytes(ctypes.byref(self.cfg), ctypes.byref(ws)))
        self._ck(self.lib.lsk_kv_pool_bytes(ctypes.byref(self.cfg), ctypes.byref(kv)))
        self._buffers.pop("sampling", None)
        self._buffers.pop("score", None)
        self._buffers["ws"] = torch.zeros(ws.value, dtype=torch.uint8, device=self.device)
        self._buffers["kv"] = torch.zeros(kv.value, dtype=torch.uint8, device=self.device)
        # MXFP4: one layer's four projections in the packed bf16 layout -- what the prefill path widens a layer's codes into
        self._buffers.pop("prefill_scratch", None)
        if self.weight_format == "mxfp4":
            hd = self.head_dim
            total = 0
            for n_rows, k in (((self.n_heads + 2 * self.n_kv_heads) * hd, self.hidden), (self.hidden, self.n_heads * hd),
                              (2 * self.intermediate, self.hidden), (self.hidden, self.intermediate)):
                nbytes = ctypes.c_size_t(0)
                self._ck(self.lib.lsk_packed_bytes(n_rows, k, ctypes.byref(nbytes)))
                total += nbytes.value
            self._buffers["prefill_scratch"] = torch.empty(total, dtype=torch.uint8, device=self.device)
        cos, sin = self._rope_tables(self.max_ctx)
        self._buffers["cos"], self._buffers["sin"] = cos, sin
        torch.cuda.synchronize(self.device)
        handle = ctypes.c_void_p(None)
        self._ck(self.lib.lsk_engine_create(ctypes.byref(self.cfg), self._buffers["ws"].data_ptr(), ws.value,
                                         self._buffers["kv"].data_ptr(), kv.value, ctypes.byref(handle)))
        self._handle = handle
        self._bind_weights()
        # a recreated engine keeps what the caller configured on the old one
        for option, value in self._options.items():
            self._ck(self.lib.lsk_engine_set_option(handle, option, value))
        if self._block_table is not None and len(self._block_table) == self.max_ctx // self.page_size:
            arr = _i32_array(self._block_table)
            self._ck(self.lib.lsk_engine_set_block_table(handle, arr, len(self._block_table), self._stream))
        else:
            self._block_table = None         # a grown pool has more pages: back to the identity mapping
        if self._profile:
            self._ck(self.lib.lsk_engine_set_profile(handle, 1))

    def _bind_weights(self) -> None:
        handle = self._handle
        if self.weight_format != "bf16":           # (the default format makes no call the parent ABI did not make)
            self._ck(self.lib.lsk_engine_set_weight_format(handle, _lib.WEIGHT_FORMATS[self.weight_format]))
        if self.weight_format == "mxfp4":
            scratch = self._buffers["prefill_scratch"]
            self._ck(self.lib.lsk_engine_set_prefill_scratch(handle, scratch.data_ptr(), scratch.numel()))
        for i, packed in enumerate(self._packed):
            if packed is None:
                continue
            wqkv, wo, wgu, wdown, n1, n2 = packed
            self._ck(self.lib.lsk_engine_set_layer(handle, i, wqkv.data_ptr(), wo.data_ptr(), wgu.data_ptr(),
                                                wdown.data_ptr(), n1.data_ptr(), n2.data_ptr()))
            if i in self._packed_prefill:           # (a recreated C engine keeps the copies _bind_prefill_copies bound)
                self._ck(self.lib.lsk_engine_set_layer_prefill(handle, i, *[t.data_ptr() for t in self._packed_prefill[i]]))
        g = self._globals
        ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731 -- NULL: not bound on this rank
        self._ck(self.lib.lsk_engine_set_globals(handle, ptr(g["embed"]), ptr(g["final_norm"]), ptr(g["lm_head"]),
                                              self._buffers["cos"].data_ptr(), self._buffers["sin"].data_ptr(), self.max_ctx))
        if self.draft_weight_format is not None:
            self.bind_draft_copies(True)

    def bind_draft_copies(self, bind: bool = True) -> None:
        """Bind (the state after construction) or unbind the draft copies of a draft_weight_format engine: unbound, its steps are the
        plain engine's.  Either way the captured step graphs are dropped (lsk_engine_set_layer_draft)."""
        if self.draft_weight_format is None:
            raise _lib.LskError("bind_draft_copies: this engine was built without draft_weight_format")
        fmt = _lib.WEIGHT_FORMATS[self.draft_weight_format]
        for i, pk in enumerate(self._packed_draft):
            ptrs = [t.data_ptr() for t in pk] if bind else [None] * 4
            self._ck(self.lib.lsk_engine_set_layer_draft(self._handle, i, fmt, *ptrs))
        self._ck(self.lib.lsk_engine_set_draft_head(self._handle, self._globals["draft_head"].data_ptr() if bind else None))

    def ensure_capacity(self, total_tokens: int, prompt_len: int) -> None:
        """Grow the KV pool / prompt buffer if a request needs more (context is lost)."""
        if total_tokens > self.max_ctx or prompt_len > self.max_prompt:
            with torch.cuda.device(self.device):
                self._allocate(max(total_tokens, self.max_ctx), max(prompt_len, self.max_prompt))

    def close(self) -> None:
        if self._handle:
            self.lib.lsk_engine_destroy(self._handle)
            self._handle = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ state
    def reset(self) -> None:
        self._ck(self.lib.lsk_engine_reset(self._handle, self._stream))

    @property
    def kv_len(self) -> int:
        v = ctypes.c_int32(0)
        self._ck(self.lib.lsk_engine_get_kv_len(self._handle, ctypes.byref(v)))
        return v.value

    def set_kv_len(self, kv_len: int) -> None:
        self._ck(self.lib.lsk_engine_set_kv_len(self._handle, int(kv_len), self._stream))

    def set_block_table(self, table: Sequence[int]) -> None:
        arr = _i32_array(table)
        self._ck(self.lib.lsk_engine_set_block_table(self._handle, arr, len(table), self._stream))
        self._block_table = [int(t) for t in table]

    # ------------------------------------------------------------------ fused fast paths
    # (each greedy / sampled pair shares one body: `fn` is its C function, `sampling` the sampled form's extra arguments)
    def _spec_step(self, fn, input_ids, num_speculations, exit_layer, eos_token_ids, sampling=()) -> StepResult:
        eos, eos_arr = self._eos_array(eos_token_ids)
        res = LskStepResult()
        self._ck(fn(self._handle, _i32_array(input_ids), len(input_ids), int(num_speculations), int(exit_layer), eos_arr, len(eos),
                    *sampling, ctypes.byref(res), self._stream))
        n, s = res.num_matches, int(num_speculations)
        return StepResult(n, res.num_drafts, res.next_token, res.kv_len, list(res.emitted[: n + 1]),
                          list(res.draft_tokens[:s]), list(res.verified_tokens[: s + 1]))

    def _spec_generate(self, fn, prompt_ids, num_speculations, exit_layer, eos_token_ids, max_steps, sampling=()):
        eos, eos_arr = self._eos_array(eos_token_ids)
        out = (ctypes.c_int32 * max_steps)()
        sd = (ctypes.c_int32 * max_steps)()
        sm = (ctypes.c_int32 * max_steps)()
        n_out, tm, td, ns = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._ck(fn(self._handle, _i32_array(prompt_ids), len(prompt_ids), int(num_speculations), int(exit_layer), eos_arr, len(eos),
                    int(max_steps), *sampling, out, ctypes.byref(n_out), ctypes.byref(tm), ctypes.byref(td), sd, sm, ctypes.byref(ns),
                    self._stream))
        steps = [(sd[i], sm[i]) for i in range(ns.value)]
        return list(out[: n_out.value]), tm.value, td.value, steps

    def _ar_generate(self, fn, input_ids, layer_end, eos_token_ids, max_steps, sampling=()) -> List[int]:
        eos, eos_arr = self._eos_array(eos_token_ids)
        out = (ctypes.c_int32 * max_steps)()
        n_out = ctypes.c_int32(0)
        self._ck(fn(self._handle, _i32_array(input_ids), len(input_ids), int(layer_end or self.num_layers), eos_arr, len(eos),
                    int(max_steps), *sampling, out, ctypes.byref(n_out), self._stream))
        return list(out[: n_out.value])

    def _ar_step(self, fn, input_ids, layer_end, sampling=()) -> int:
        tok = ctypes.c_int32(0)
        self._ck(fn(self._handle, _i32_array(input_ids), len(input_ids), int(layer_end or self.num_layers), *sampling,
                    ctypes.byref(tok), self._stream))
        return tok.value

    def spec_step(self, input_ids: Sequence[int], num_speculations: int, exit_layer: int,
                  eos_token_ids: Sequence[int]) -> StepResult:
        return self._spec_step(self.lib.lsk_spec_step, input_ids, num_speculations, exit_layer, eos_token_ids)

    def spec_generate(self, prompt_ids: Sequence[int], num_speculations: int, exit_layer: int,
                      eos_token_ids: Sequence[int], max_steps: int):
        """Whole greedy generation in one C-ABI call.  Returns (tokens, matches, drafts, [(T_d, n) per step])."""
        return self._spec_generate(self.lib.lsk_spec_generate, prompt_ids, num_speculations, exit_layer, eos_token_ids, max_steps)

    # ------------------------------------------------------------------ sampling on the device (opt-in)
    def _sampling_scratch(self) -> torch.Tensor:
        self._check_device_sampling()
        buf = self._buffers.get("sampling")
        if buf is None:
            n = ctypes.c_size_t(0)
            self._ck(self.lib.lsk_sampling_scratch_bytes(ctypes.byref(self.cfg), ctypes.byref(n)))
            buf = torch.empty(n.value, dtype=torch.uint8, device=self.device)
            self._buffers["sampling"] = buf
        return buf

    def _check_device_sampling(self) -> None:
        if not self.samples_on_device:
            raise _lib.LskError(f"the {self.dtype} engine does not sample on the device (16-bit sampler keys); sample=True runs on the host path")

    def _sampling_args(self, temperature, top_k, top_p, seed, offset) -> tuple:
        """The sample=True arguments of a sampled entry point: warping, Philox key and counter, the sampling scratch."""
        scratch = self._sampling_scratch()
        return (float(temperature), int(top_k), float(top_p), _u64(seed), _u64(offset), scratch.data_ptr(), scratch.numel())

    def sample_rows(self, logits: torch.Tensor, temperature: float, top_k: int, top_p: float, seed: int, offset: int,
                    tag0: int = 0):
        """decode_next_token(sample=True) over rows of device logits [m, ld] (fp32).  Returns (tokens int32[m] on
        the device, probabilities fp32 [m, ld])."""
        self._check_device_sampling()
        if logits.dtype != torch.float32 or logits.device != self.device or logits.dim() != 2 or logits.stride(1) != 1:
            raise _lib.LskError("logits must be a [m, ld] fp32 tensor on the engine device")
        m, ld = logits.shape[0], logits.stride(0)
        toks = torch.empty(m, dtype=torch.int32, device=self.device)
        probs = torch.empty(m, ld, dtype=torch.float32, device=self.device)
        self._ck(self.lib.lsk_sample_rows(self._handle, logits.data_ptr(), ld, m, float(temperature), int(top_k), float(top_p),
                                       _u64(seed), _u64(offset), int(tag0), toks.data_ptr(), probs.data_ptr(), self._stream))
        return toks, probs

    def spec_step_sampled(self, input_ids: Sequence[int], num_speculations: int, exit_layer: int,
                          eos_token_ids: Sequence[int], temperature: float, top_k: int, top_p: float, seed: int,
                          offset: int) -> StepResult:
        """single_step_speculation with sample=True, entirely on the device (lsk_spec_step_sampled)."""
        return self._spec_step(self.lib.lsk_spec_step_sampled, input_ids, num_speculations, exit_layer, eos_token_ids,
                               self._sampling_args(temperature, top_k, top_p, seed, offset))

    def spec_generate_sampled(self, prompt_ids: Sequence[int], num_speculations: int, exit_layer: int,
                              eos_token_ids: Sequence[int], max_steps: int, temperature: float, top_k: int, top_p: float,
                              seed: int, offset: int):
        """Whole sample=True generation in one C-ABI call (lsk_spec_generate_sampled).  Same return as spec_generate."""
        return self._spec_generate(self.lib.lsk_spec_generate_sampled, prompt_ids, num_speculations, exit_layer, eos_token_ids, max_steps,
                                   self._sampling_args(temperature, top_k, top_p, seed, offset))

    def ar_generate(self, input_ids: Sequence[int], layer_end: Optional[int], eos_token_ids: Sequence[int],
                    max_steps: int) -> List[int]:
        """Whole greedy autoregressive generation in one C-ABI call."""
        return self._ar_generate(self.lib.lsk_ar_generate, input_ids, layer_end, eos_token_ids, max_steps)

    def ar_step(self, input_ids: Sequence[int], layer_end: Optional[int] = None) -> int:
        return self._ar_step(self.lib.lsk_ar_step, input_ids, layer_end)

    def ar_generate_sampled(self, input_ids: Sequence[int], layer_end: Optional[int], eos_token_ids: Sequence[int], max_steps: int,
                            temperature: float, top_k: int, top_p: float, seed: int, offset: int) -> List[int]:
        """Whole sample=True autoregressive generation in one C-ABI call (lsk_ar_generate_sampled): token i draws at Philox
        counter offset + i, the draw step i of spec_generate_sampled makes with num_speculations = 0."""
        return self._ar_generate(self.lib.lsk_ar_generate_sampled, input_ids, layer_end, eos_token_ids, max_steps,
                                 self._sampling_args(temperature, top_k, top_p, seed, offset))

    def ar_step_sampled(self, input_ids: Sequence[int], layer_end: Optional[int], temperature: float, top_k: int, top_p: float,
                        seed: int, offset: int) -> int:
        """One sample=True autoregressive token (lsk_ar_step_sampled), drawn at Philox counter `offset`; only the id comes back."""
        return self._ar_step(self.lib.lsk_ar_step_sampled, input_ids, layer_end,
                             self._sampling_args(temperature, top_k, top_p, seed, offset))

    # ------------------------------------------------------------------ layer-range pipeline (rank-0 half of a step)
    def draft_block(self, input_ids: Optional[Sequence[int]], row0: int, n_rows: int, pos_off0: int, exit_layer: int,
                    head_last: bool = False) -> None:
        """Asynchronous device-resident draft loop over step rows [row0, row0 + n_rows) (lsk_draft_block)."""
        self._ck(self.lib.lsk_draft_block(self._handle, *_host_ids(input_ids), int(row0), int(n_rows), int(pos_off0), int(exit_layer),
                                       1 if head_last else 0, self._stream))

    def set_eos(self, eos_token_ids: Sequence[int]) -> None:
        """The eos list of the acceptance kernel (pipeline ranks: lsk_engine_set_eos)."""
        eos, arr = self._eos_array(eos_token_ids)
        self._ck(self.lib.lsk_engine_set_eos(self._handle, arr, len(eos), self._stream))

    def pipeline_pack(self, go: int, prompt_len: int, src_row: int, m: int, kv: int) -> None:
        """Rank 0: step rows [src_row, src_row + m) + header -> the message buffer (lsk_pipeline_pack), asynchronous."""
        self._ck(self.lib.lsk_pipeline_pack(self._handle, int(go), int(prompt_len), int(src_row), int(m), int(kv), self._stream))

    def pipeline_apply(self, kv_bound: int) -> None:
        """Ranks > 0: the received header's rollback applied on the device; the host keeps `kv_bound` (lsk_pipeline_apply)."""
        self._ck(self.lib.lsk_pipeline_apply(self._handle, int(min(kv_bound, self.max_ctx)), self._stream))

    def pipeline_tail(self, m: int) -> torch.Tensor:
        """Last rank: head + argmax + acceptance kernel over message rows [1, 1 + m) -> device int32[64] result block."""
        res = self._buffers.get("pp_result")
        if res is None:
            res = torch.zeros(64, dtype=torch.int32, device=self.device)
            self._buffers["pp_result"] = res
        self._ck(self.lib.lsk_pipeline_tail(self._handle, int(m), res.data_ptr(), self._stream))
        return res

    # ---- sample=True on the pipeline (lsk_draft_block_sampled / lsk_pipeline_pack_sampled / _tail_sampled / _residual) ----
    def pipeline_result_words(self) -> int:
        """int32 words of a sampled step's result block: 64 result words + one fp32 probability row (q_n)."""
        n = ctypes.c_int32(0)
        self._ck(self.lib.lsk_pipeline_result_words(ctypes.byref(self.cfg), ctypes.byref(n)))
        return n.value

    def draft_block_sampled(self, input_ids: Optional[Sequence[int]], row0: int, n_rows: int, pos_off0: int, exit_layer: int,
                            head_last: bool, temperature: float, top_k: int, top_p: float, seed: int, offset: int) -> None:
        """`draft_block` with every argmax replaced by a draw (draft j of the block: Philox tag j at `offset`); the warped draft
        distributions stay in the sampling scratch (rows row0 + j) for `pipeline_pack_sampled` / `pipeline_residual`."""
        self._ck(self.lib.lsk_draft_block_sampled(self._handle, *_host_ids(input_ids), int(row0), int(n_rows), int(pos_off0),
                                               int(exit_layer), 1 if head_last else 0,
                                               *self._sampling_args(temperature, top_k, top_p, seed, offset), self._stream))

    def pipeline_pack_sampled(self, go: int, prompt_len: int, src_row: int, m: int, kv: int, offset: int) -> None:
        """`pipeline_pack` + the sampled step's header words: mode, Philox offset, p_i(x_i) of every draft."""
        scratch = self._sampling_scratch()
        self._ck(self.lib.lsk_pipeline_pack_sampled(self._handle, int(go), int(prompt_len), int(src_row), int(m), int(kv), _u64(offset),
                                                 scratch.data_ptr(), scratch.numel(), self._stream))

    def pipeline_tail_sampled(self, m: int, temperature: float, top_k: int, top_p: float, seed: int, offset: int) -> torch.Tensor:
        """Last rank, sample=True: head + verify draws + the acceptance test against the header's p_i(x_i) -> device int32
        [pipeline_result_words()] = result words + the verify row q_n at the first rejection."""
        words = self.pipeline_result_words()
        res = self._buffers.get("pp_result_sampled")
        if res is None or res.numel() != words:
            res = torch.zeros(words, dtype=torch.int32, device=self.device)
            self._buffers["pp_result_sampled"] = res
        self._ck(self.lib.lsk_pipeline_tail_sampled(self._handle, int(m), *self._sampling_args(temperature, top_k, top_p, seed, offset),
                                                 res.data_ptr(), words, self._stream))
        return res

    def pipeline_residual(self, block: torch.Tensor, src_row: int, seed: int, offset: int) -> None:
        """Rank 0: finish a sampled result block in place -- if its residual draw is pending, the token from max(q_n - p_n, 0) with
        this rank's p_n (the draft rows start at step row `src_row`)."""
        if block.dtype != torch.int32 or block.device != self.device or not block.is_contiguous():
            raise _lib.LskError("the result block must be a contiguous int32 tensor on the engine device")
        scratch = self._sampling_scratch()
        self._ck(self.lib.lsk_pipeline_residual(self._handle, block.data_ptr(), block.numel(), int(src_row), _u64(seed), _u64(offset),
                                             scratch.data_ptr(), scratch.numel(), self._stream))

    # ------------------------------------------------------------------ scoring (lsk_score.h)
    def _score_scratch(self) -> torch.Tensor:
        buf = self._buffers.get("score")
        if buf is None:
            n = ctypes.c_size_t(0)
            self._ck(self.lib.lsk_score_scratch_bytes(ctypes.byref(self.cfg), ctypes.byref(n)))
            buf = torch.empty(n.value, dtype=torch.uint8, device=self.device)
            self._buffers["score"] = buf
        return buf

    def score_rows(self, logits: torch.Tensor, targets: torch.Tensor):
        """Log-probability of ``targets[r]`` under row r of device logits [m, ld] (fp32, m <= 16) and the row's argmax (lowest index
        on ties).  Returns (logprob fp32[m], argmax int32[m]) on the device; columns >= vocab of a row are never read."""
        if logits.dtype != torch.float32 or logits.device != self.device or logits.dim() != 2 or logits.stride(1) != 1:
            raise _lib.LskError("logits must be a [m, ld] fp32 tensor on the engine device")
        m, ld = logits.shape[0], (logits.stride(0) if logits.shape[0] > 1 else max(logits.stride(0), logits.shape[1]))
        if targets.dtype != torch.int32 or targets.device != self.device or targets.shape != (m,) or not targets.is_contiguous():
            raise _lib.LskError("targets must be a contiguous int32 tensor [m] on the engine device")
        scratch = self._score_scratch()
        lp = torch.empty(m, dtype=torch.float32, device=self.device)
        am = torch.empty(m, dtype=torch.int32, device=self.device)
        self._ck(self.lib.lsk_score_rows(self._handle, logits.data_ptr(), ld, m, targets.data_ptr(), lp.data_ptr(), am.data_ptr(),
                                      scratch.data_ptr(), scratch.numel(), self._stream))
        return lp, am

    def score(self, ids: Sequence[int], layer_ends: Optional[Sequence[int]] = None) -> ScoreResult:
        """Teacher-forced scores of ``ids`` (n >= 2) at the exit layers ``layer_ends`` (strictly increasing, at most 8; default: the
        whole model) in one call: one prefill, then every position's head scored against the next id on the device (lsk_score).
        The cached context is dropped; kv_len is 0 afterwards."""
        ids = [int(t) for t in ids]
        ends = [int(e) for e in (layer_ends if layer_ends is not None else [self.num_layers])]
        n = len(ids)
        if n < 2:
            raise _lib.LskError("score: at least two ids (a context token and a target)")
        self.ensure_capacity(n - 1, n - 1)
        scratch = self._score_scratch()
        lp = torch.empty(max(1, len(ends)), n - 1, dtype=torch.float32)
        am = torch.empty(max(1, len(ends)), n - 1, dtype=torch.int32)
        self._ck(self.lib.lsk_score(self._handle, _i32_array(ids), n, _i32_array(ends), len(ends),
                                 ctypes.cast(lp.data_ptr(), ctypes.POINTER(ctypes.c_float)),
                                 ctypes.cast(am.data_ptr(), ctypes.POINTER(ctypes.c_int32)),
                                 scratch.data_ptr(), scratch.numel(), self._stream))
        return ScoreResult(ids, ends, lp[: len(ends)], am[: len(ends)])

    def logits_rows(self, blocks: Sequence[Sequence[int]]) -> torch.Tensor:
        """Final norm + lm_head logits of the listed (buffer, row_base, count) blocks -> [rows, vocab] in the model dtype (the values
        the reference's `model.lm_head` returns, LMU:273, :387): what logits processors are shown."""
        total = sum(c for _, _, c in blocks)
        # (16 rows at a time through ONE fp32 staging block straight into the model dtype: a 2 048-row prompt at V = 128 256 is 0.5 GB in
        # bf16; the fp32 image of all rows plus a converted copy was three times that)
        out = torch.empty(total, self.vocab, dtype=self.dtype, device=self.device)
        stage = torch.empty(_lib.LSK_MAX_ROWS, self.vocab, dtype=torch.float32, device=self.device)
        at = 0
        for buf, base, count in blocks:
            for r0 in range(0, count, _lib.LSK_MAX_ROWS):
                m = min(_lib.LSK_MAX_ROWS, count - r0)
                self.run_head(buf, base + r0, m, logits=stage[:m], want_tokens=False)
                out[at:at + m].copy_(stage[:m])
                at += m
        return out

    def header(self) -> List[int]:
        """The int32 words of the message header (synchronises: a device -> host read)."""
        return [int(v) for v in self.rows_view(BUF_MSG, 0, 1).view(torch.int32)[0, :24].tolist()]

    def row_tokens(self, row0: int, n: int) -> List[int]:
        out = (ctypes.c_int32 * n)()
        self._ck(self.lib.lsk_get_row_tokens(self._handle, int(row0), int(n), out, self._stream))
        return list(out)

    def shift_rows(self, src: int, dst: int, n: int) -> None:
        self._ck(self.lib.lsk_shift_rows(self._handle, int(src), int(dst), int(n), self._stream))

    def rows_view(self, buffer: int, row_base: int, m: int) -> torch.Tensor:
        """Rows of a hidden-state buffer as a ZERO-COPY tensor over the engine's workspace ([m, hidden], model dtype):
        point-to-point send / recv go straight from / into the engine's buffers on the current stream."""
        off = ctypes.c_size_t(0)
        self._ck(self.lib.lsk_rows_offset(self._handle, buffer, row_base, ctypes.byref(off)))
        nbytes = m * self.hidden * self.elem_bytes
        return self._buffers["ws"][off.value: off.value + nbytes].view(self.dtype).view(m, self.hidden)

    # ------------------------------------------------------------------ building blocks
    def embed_rows(self, ids: Sequence[int], buffer: int, row_base: int) -> None:
        arr = _i32_array(ids)
        self._ck(self.lib.lsk_embed_rows(self._handle, arr, len(ids), buffer, row_base, self._stream))

    def run_layers(self, buffer: int, row_base: int, m: int, pos_offset: int, layer_begin: int, layer_end: int) -> None:
        self._ck(self.lib.lsk_run_layers(self._handle, buffer, row_base, m, pos_offset, layer_begin, layer_end, self._stream))

    def run_layers_chunked(self, buffer: int, row_base: int, n: int, pos_offset: int, layer_begin: int, layer_end: int) -> None:
        for r0 in range(0, n, _lib.LSK_MAX_ROWS):
            m = min(_lib.LSK_MAX_ROWS, n - r0)
            self.run_layers(buffer, row_base + r0, m, pos_offset + r0, layer_begin, layer_end)

    def run_bulk(self, n: int, layer_begin: int, layer_end: int) -> None:
        self._ck(self.lib.lsk_run_bulk(self._handle, n, layer_begin, layer_end, self._stream))

    def set_option(self, option: int, value: int) -> None:
        self._ck(self.lib.lsk_engine_set_option(self._handle, option, value))
        self._options[int(option)] = int(value)

    def run_head(self, buffer: int, row_base: int, m: int, logits: Optional[torch.Tensor] = None,
                 want_tokens: bool = True) -> Optional[List[int]]:
        """logits: optional fp32 CUDA tensor [m, >=vocab] that receives the (bf16-rounded) logits."""
        ptr, ld = None, 0
        if logits is not None:
            if logits.dtype != torch.float32 or logits.device != self.device or logits.stride(-1) != 1:
                raise _lib.LskError("logits buffer must be a contiguous fp32 tensor on the engine device")
            ptr, ld = logits.data_ptr(), logits.stride(0)
        toks = (ctypes.c_int32 * m)() if want_tokens else None
        self._ck(self.lib.lsk_run_head(self._handle, buffer, row_base, m, ptr, ld, toks, self._stream))
        return list(toks) if want_tokens else None

    def read_rows(self, buffer: int, row_base: int, m: int) -> torch.Tensor:
        out = torch.empty(m, self.hidden, dtype=self.dtype, device=self.device)
        self._ck(self.lib.lsk_read_rows(self._handle, buffer, row_base, m, out.data_ptr(), self._stream))
        return out

    def write_rows(self, buffer: int, row_base: int, rows: torch.Tensor) -> None:
        rows = rows.to(self.device, self.dtype).contiguous()
        self._ck(self.lib.lsk_write_rows(self._handle, buffer, row_base, rows.shape[0], rows.data_ptr(), self._stream))

    # ------------------------------------------------------------------ measurement hooks
    def time_gateup(self, layer: int, m: int, iters: int) -> float:
        ms = ctypes.c_float(0.0)
        self._ck(self.lib.lsk_time_gateup(self._handle, layer, m, iters, ctypes.byref(ms), self._stream))
        return ms.value

    def set_profile(self, enable: bool) -> None:
        self._ck(self.lib.lsk_engine_set_profile(self._handle, 1 if enable else 0))
        self._profile = bool(enable)

    def get_profile(self):
        """(sum of the gate/up dispatch durations in ms, number of launches)."""
        ms, n = ctypes.c_float(0.0), ctypes.c_int32(0)
        self._ck(self.lib.lsk_engine_get_profile(self._handle, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def host_stats(self) -> dict:
        """Host cost of the fused generate calls since the last query (lsk_engine_get_host_stats)."""
        a, b, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
        self._ck(self.lib.lsk_engine_get_host_stats(self._handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return {"enqueue_s": a.value, "wall_s": b.value, "steps": n.value}

    PROFILE_CLASSES = ("qkv", "attention", "o_proj", "gate_up", "down", "lm_head")

    def get_profile_table(self):
        """[{kernel, rows ("1" | ">1"), launches, ms, bytes}] for every decode-path kernel class since set_profile(True)."""
        n = 2 * len(self.PROFILE_CLASSES)
        ms, cnt, by = (ctypes.c_float * n)(), (ctypes.c_int32 * n)(), (ctypes.c_double * n)()
        self._ck(self.lib.lsk_engine_get_profile_table(self._handle, n, ms, cnt, by))
        out = []
        for c, name in enumerate(self.PROFILE_CLASSES):
            for multi in (0, 1):
                i = 2 * c + multi
                if cnt[i]:
                    out.append({"kernel": name, "rows": ">1" if multi else "1", "launches": cnt[i], "ms": ms[i], "bytes": by[i]})
        return out

    # bytes one launch of each projection streams from HBM (algorithmic: the packed weights once)
    def projection_bytes(self, weight_format: Optional[str] = None) -> dict:
        """`weight_format`: another format's bytes for this geometry (the draft copies'); default: the engine's own."""
        wf = weight_format or self.weight_format
        hd = self.head_dim
        qdim, kvdim = self.n_heads * hd, self.n_kv_heads * hd
        eb = self.elem_bytes
        fp8_size = lambda n, k: _round_up(n, 16) * (k + 4)       # noqa: E731 -- 1-byte codes + one fp32 power of two per packed row
        if wf == "fp8_e4m3":    # (the lm_head's rows pad to a whole tile)
            size = fp8_size
        elif wf == "mxfp4":     # 4-bit codes + the exponent table (a row padded to whole dwords, 16 bytes behind it)
            size = lambda n, k: _round_up(n, 16) * (k // 2 + _round_up(k // 32, 4)) + 16       # noqa: E731
        else:
            size = lambda n, k: eb * n * k                         # noqa: E731
        head_size = fp8_size if wf == "mxfp4" else size
        return {
            "qkv": size(qdim + 2 * kvdim, self.hidden),
            "o": size(self.hidden, qdim),
            "gate_up": size(2 * self.intermediate, self.hidden),
            "down": size(self.hidden, self.intermediate),
            "lm_head": head_size(self.vocab, self.hidden),
        }


_ENGINES = None


def get_engine(model, check_weights: bool = True, **kwargs) -> HipEngine:
    """The engine bound to ``model`` (built lazily on first use, reused across calls).  Kept in a weak
    map, not on the module, so ``copy.deepcopy(model)`` and ``state_dict()`` never see it.

    The engine streams PACKED COPIES of the projections, so it must notice when the model's weights change under it
    (load_state_dict, an in-place edit, a LoRA merge on the same object -- the reference always reads live weights):
    with ``check_weights`` the fingerprint taken at pack time -- (address, version) per tensor plus a sampled content
    checksum, which is what catches edits through ``.data`` -- is compared and the weights are re-packed on a mismatch.  Keyword arguments that differ from the cached engine's are applied where that is possible
    (capacity grows, target_wgs is an option) and reported otherwise."""
    global _ENGINES
    if _ENGINES is None:
        import weakref
        _ENGINES = weakref.WeakKeyDictionary()
    # one engine per (model, weight format): a request for one format is never served by an engine of the other
    fmt = kwargs.get("weight_format") or "bf16"
    if kwargs.get("draft_weight_format"):        # ... and per draft format and depth; without the option the key is what it was
        fmt = (fmt, kwargs["draft_weight_format"], kwargs.get("draft_layers"))
    per_model = _ENGINES.get(model)
    if per_model is None:
        per_model = _ENGINES[model] = {}
    eng = per_model.get(fmt)
    if eng is None:
        eng = HipEngine(model, **kwargs)
        per_model[fmt] = eng
        return eng
    if check_weights and eng.weights_changed(model):
        eng.refresh_weights(model)
    if kwargs:
        import warnings
        if kwargs.get("max_ctx", 0) > eng.max_ctx or kwargs.get("max_prompt", 0) > eng.max_prompt:
            eng.ensure_capacity(kwargs.get("max_ctx", eng.max_ctx), kwargs.get("max_prompt", eng.max_prompt))
        tw = kwargs.get("target_wgs")
        if tw is not None and tw != eng.target_wgs:
            eng.target_wgs = tw
            eng.set_option(_lib.LSK_OPT_TARGET_WGS, tw)
        for key in ("release_weights", "layer_range", "page_size"):
            if key in kwargs and kwargs[key] is not None:
                have = getattr(eng, key)
                want = tuple(kwargs[key]) if key == "layer_range" else kwargs[key]
                if have != want:
                    warnings.warn(f"get_engine: {key}={kwargs[key]!r} ignored, the engine cached for this model was built "
                                  f"with {key}={have!r}", RuntimeWarning, stacklevel=2)
    return eng
