"""Text generation (capability parity with reference
src/modalities/inference/text/inference_component.py:11-105): prompt
templating, temperature/argmax sampling, incremental decode printing.

MI355X-first improvement over the reference: a KV-cache-free full-context
re-forward per token is kept as the simple default (matching the reference's
behavior) but generation batches the forward on device in bf16.

With a KV cache on the GPU, the per-token decode step reads its position
from device counters (KVCache.pos_dev), so after the prefill one step is
captured into a hipGraph (`DecodeGraph`) and replayed per token: the eager
launch chain of a step is paid once. `use_decode_graph=False` opts out; a
capture that fails falls back to the eager step.

`decode_weight_format` ("fp8_e4m3" or "bf16"; default None = off) has the
model build its decode weights (GPT2LLM.prepare_decode_weights) before the
prefill: the single-token steps, captured or eager, then run their linears
through the in-tree skinny GEMM, on weight-only FP8 for "fp8_e4m3"."""

import sys
from typing import Optional

import torch

from modalities_amd.tokenization.tokenizer_wrapper import TokenizerWrapper


class DecodeGraph:
    """One single-token `model.forward_cached` step on `cache`, captured
    into a hipGraph after the prefill and replayed per token.

    Static buffers: `ids` [B, 1] (write the next token here) and `logits`
    [B, 1, V] (valid after `step`). Single stream; one warm-up step runs on
    a side stream first and is then undone (the cache row it wrote is the
    one the first replay rewrites). The host mirror cache.pos is advanced
    per replay; the device counters advance inside the graph."""

    def __init__(self, model, cache, sample_key: str, prediction_key: str):
        self.cache = cache
        self.sample_key = sample_key
        dev = cache.pos_dev.device
        B = cache.pos_dev.shape[0]
        self.ids = torch.zeros(B, 1, dtype=torch.long, device=dev)
        pos = cache.pos
        if pos + 1 > cache.max_len:
            raise ValueError("KV cache is full: nothing left to decode")

        def rewind():
            cache.pos = pos
            cache.pos_dev.fill_(pos)

        try:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                model.forward_cached({sample_key: self.ids}, cache)
            torch.cuda.current_stream(dev).wait_stream(side)
            rewind()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.logits = model.forward_cached(
                    {sample_key: self.ids}, cache)[prediction_key]
        finally:
            rewind()

    def step(self, next_ids: torch.Tensor) -> torch.Tensor:
        """Decode one token per row; returns the static logits [B, 1, V]."""
        if self.cache.pos + 1 > self.cache.max_len:
            raise ValueError(f"KV cache overflow: {self.cache.pos}+1 > "
                             f"{self.cache.max_len}")
        self.ids.copy_(next_ids)
        self.graph.replay()
        self.cache.pos += 1
        return self.logits


def capture_decode_graph(model, cache, sample_key: str = "input_ids",
                         prediction_key: str = "logits"
                         ) -> Optional[DecodeGraph]:
    """A DecodeGraph when the model decodes on the GPU through the decode
    kernels and the capture succeeds; None (decode eagerly) otherwise."""
    route = getattr(model, "_decode_route", None)
    if route is None or not cache.pos_dev.is_cuda \
            or not route(cache.pos_dev):
        return None
    try:
        return DecodeGraph(model, cache, sample_key, prediction_key)
    except Exception as e:
        print(f"# hipGraph capture of the decode step unavailable "
              f"({type(e).__name__}: {e}); decoding eagerly",
              file=sys.stderr, flush=True)
        return None


class TextInferenceComponent:
    def __init__(self, model, tokenizer: TokenizerWrapper, prompt_template: str,
                 sequence_length: int, temperature: float = 1.0,
                 eod_token: str = "<eod>", device: Optional[torch.device] = None,
                 sample_key: str = "input_ids", prediction_key: str = "logits",
                 top_k: Optional[int] = None, top_p: Optional[float] = None,
                 use_decode_graph: bool = True,
                 decode_weight_format: Optional[str] = None):
        if decode_weight_format is not None \
                and not hasattr(model, "prepare_decode_weights"):
            raise ValueError(
                f"decode_weight_format={decode_weight_format!r}: "
                f"{type(model).__name__} has no prepare_decode_weights")
        self.model = model
        self.tokenizer = tokenizer
        self.prompt_template = prompt_template
        self.sequence_length = sequence_length
        self.temperature = temperature
        self.eod_token = eod_token
        self.device = device or torch.device("cpu")
        self.sample_key = sample_key
        self.prediction_key = prediction_key
        self.top_k = top_k
        self.top_p = top_p
        self.use_decode_graph = use_decode_graph
        self.decode_weight_format = decode_weight_format

    def _sample(self, logits: torch.Tensor) -> torch.Tensor:
        """Greedy (temperature==0) or temperature sampling with optional
        top-k / nucleus (top-p) filtering."""
        if self.temperature <= 0:
            return logits.argmax(dim=-1, keepdim=True)
        logits = logits / self.temperature
        if self.top_k is not None and self.top_k > 0:
            kth = torch.topk(logits, min(self.top_k, logits.shape[-1]),
                             dim=-1).values[..., -1:]
            logits = logits.masked_fill(logits < kth, float("-inf"))
        if self.top_p is not None and 0.0 < self.top_p < 1.0:
            sorted_logits, sorted_idx = torch.sort(logits, descending=True,
                                                   dim=-1)
            cum = torch.softmax(sorted_logits, dim=-1).cumsum(-1)
            # drop tokens whose EXCLUSIVE cumulative prob already exceeds
            # top_p (the highest-prob token always stays)
            drop_sorted = torch.zeros_like(cum, dtype=torch.bool)
            drop_sorted[..., 1:] = cum[..., :-1] > self.top_p
            drop = torch.zeros_like(drop_sorted).scatter(
                -1, sorted_idx, drop_sorted)
            logits = logits.masked_fill(drop, float("-inf"))
        probs = torch.softmax(logits, dim=-1)
        return torch.multinomial(probs, num_samples=1)

    @torch.no_grad()
    def generate_tokens(self, context: str, echo: bool = False) -> str:
        """Greedy (temperature==0) or temperature sampling until eod or
        sequence_length tokens."""
        ids = self.tokenizer.tokenize(context)
        input_ids = torch.tensor(ids, dtype=torch.long,
                                 device=self.device).unsqueeze(0)
        try:
            eod_id = self.tokenizer.get_token_id(self.eod_token)
        except Exception:
            eod_id = None
        generated: list[int] = []
        max_new = max(0, self.sequence_length - input_ids.shape[1])
        self.model.eval()
        if self.decode_weight_format is not None and getattr(
                self.model, "decode_weight_format",
                None) != self.decode_weight_format:
            self.model.prepare_decode_weights(self.decode_weight_format)

        # KV-cache incremental decode when the model supports it (GPT2LLM);
        # fall back to full-context re-forward otherwise.
        cache = None
        if hasattr(self.model, "forward_cached") and                 hasattr(self.model, "new_kv_cache"):
            cache = self.model.new_kv_cache(input_ids.shape[0],
                                            max_len=self.sequence_length)
            out = self.model.forward_cached({self.sample_key: input_ids}, cache)
        else:
            out = self.model({self.sample_key: input_ids})

        graph = None
        graph_tried = not (self.use_decode_graph and cache is not None)
        for i in range(max_new):
            logits = out[self.prediction_key][:, -1, :].float()
            next_id = self._sample(logits)
            token = next_id.item()
            if eod_id is not None and token == eod_id:
                break
            generated.append(token)
            if echo:
                sys.stdout.write(self.tokenizer.decode([token]))
                sys.stdout.flush()
            if i + 1 >= max_new:
                break
            if cache is not None:
                if cache.pos >= self.sequence_length:
                    break
                if not graph_tried:   # after the prefill, before step 1
                    graph_tried = True
                    graph = capture_decode_graph(
                        self.model, cache, self.sample_key,
                        self.prediction_key)
                if graph is not None:
                    out = {self.prediction_key: graph.step(next_id)}
                else:
                    out = self.model.forward_cached(
                        {self.sample_key: next_id}, cache)
            else:
                input_ids = torch.cat([input_ids, next_id], dim=1)
                out = self.model({self.sample_key: input_ids})
        if echo:
            sys.stdout.write("\n")
        return self.tokenizer.decode(generated)

    def run(self) -> None:
        """Interactive prompt loop (reference inference_component.py:90-105)."""
        while True:
            try:
                prompt = input("enter prompt> ")
            except (EOFError, KeyboardInterrupt):
                break
            if not prompt.strip():
                continue
            text = self.prompt_template.format(text=prompt) \
                if "{text}" in self.prompt_template else prompt
            self.generate_tokens(text, echo=True)
