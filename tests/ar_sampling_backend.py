"""CPU model of the sampled autoregressive entry points (tests only): CpuStageBackend's arithmetic plus the oracle's draw-for-draw
model of the sampling kernels (oracle/sampling_oracle.py), orchestrated as lsk_ar_step_sampled / lsk_ar_generate_sampled do it
(csrc/lsk_generate.hip): token i is the draw over its logits row at Philox counter offset + i with the verify tag."""
import torch

from cpu_stage_backend import CpuStageBackend


class ArSampledCpuBackend(CpuStageBackend):
    def ar_step_sampled(self, input_ids, layer_end, temperature, top_k, top_p, seed, offset):
        from oracle import sampling_oracle as so
        ids = [int(t) for t in input_ids]
        P, le = len(ids), int(layer_end or self.num_layers)
        if P > 1:
            self.embed_rows(ids[:-1], 1, 0)
            self.run_bulk(P - 1, 0, le)
        self.embed_rows(ids[-1:], 0, 0)
        self.run_layers(0, 0, 1, P - 1, 0, le)
        tok, _ = so.device_sample_row(self._logits_np(0, 0, 1)[0], temperature, top_k, top_p, seed, offset, so.TAG_VERIFY)
        self.set_kv_len(self.kv_len + P)
        return int(tok)

    def ar_generate_sampled(self, input_ids, layer_end, eos_token_ids, max_steps, temperature, top_k, top_p, seed, offset):
        self.reset()
        cur, out = [int(t) for t in input_ids], []
        for i in range(max_steps):
            tok = self.ar_step_sampled(cur, layer_end, temperature, top_k, top_p, seed, offset + i)
            if tok in eos_token_ids:
                break
            out.append(tok)
            cur = [tok]
        self.set_kv_len(len(input_ids) + max(len(out) - 1, 0))       # lsk_ar_generate's final context length
        return out


class RecordingArBackend(ArSampledCpuBackend):
    """Records the entry points a strategy calls; logits materialised OUTSIDE the sampled entry points count as host sampling."""

    def __init__(self, model, layer_range=None):
        super().__init__(model, layer_range=layer_range)
        self.calls = []
        self._inside = 0

    def run_head(self, buffer, row_base, m, logits=None, want_tokens=True):
        if not self._inside:
            self.calls.append(("run_head", m))
        return super().run_head(buffer, row_base, m, logits=logits, want_tokens=want_tokens)

    def ar_step_sampled(self, input_ids, layer_end, temperature, top_k, top_p, seed, offset):
        if not self._inside:
            self.calls.append(("ar_step_sampled", list(input_ids), layer_end, temperature, top_k, top_p, seed, offset))
        self._inside += 1
        try:
            return super().ar_step_sampled(input_ids, layer_end, temperature, top_k, top_p, seed, offset)
        finally:
            self._inside -= 1

    def ar_generate_sampled(self, input_ids, layer_end, eos_token_ids, max_steps, temperature, top_k, top_p, seed, offset):
        self.calls.append(("ar_generate_sampled", list(input_ids), layer_end, list(eos_token_ids), max_steps, temperature, top_k, top_p,
                           seed, offset))
        self._inside += 1
        try:
            with torch.inference_mode():
                return super().ar_generate_sampled(input_ids, layer_end, eos_token_ids, max_steps, temperature, top_k, top_p, seed, offset)
        finally:
            self._inside -= 1

    def names(self):
        return [c[0] for c in self.calls]
