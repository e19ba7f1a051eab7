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

`decode_weight_format` ("fp8_e4m3", "bf16" or "mxfp4"; default None = off) has the
model build its decode weights (GPT2LLM.prepare_decode_weights) before the
prefill: the single-token steps of a batch of at most 32, captured or eager,
then run their linears through the in-tree skinny GEMMs (the VALU kernel up
to batch 8, the MFMA kernel for batch 9..32), on weight-only FP8 for
"fp8_e4m3"; "mxfp4" runs every such batch through the MXFP4 MFMA kernel on
4-bit microscaled weights (0.53 bytes per weight).

`kv_cache_format` ("fp8_e4m3"; default None = a cache in the model's dtype)
has the model allocate an e4m3 KV cache (GPT2LLM.new_kv_cache(kv_format=...)):
0.5x + 4 bytes per cached row, read by the FP8 decode kernels; the prefill
stores quantised. It pays where the cache, not the weights, is the traffic:
large batch times long context (profiles/decode_attention.md).

`prefill_chunk_tokens` (an integer >= 2; default None = the prompt in one
piece) feeds a longer prompt to `forward_cached` in chunks of that many
tokens: the first chunk takes the prefill kernel, the later ones attend over
the cache in place through `ops.decode_attention` (for the duration of the
prefill `ops.decode_chunk_tokens()` is raised to at least the chunk size),
which bounds the activation memory of a long prompt. With an FP8 cache a
chunk reads its own rows quantised.

`device_sampling=True` (default off) samples with `ops.sample_logits`: one
HIP kernel for temperature, top-k, top-p and the draw, reading the logits
where lm_head left them. A captured decode step then ends in `torch.rand`
and that kernel, which writes the next id into the graph's own input
buffer: between two replays the host only reads the id back for the eod
check (profiles/sampling.md)."""

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
    per replay; the device counters advance inside the graph.

    With `sampler` = (temperature, top_k, top_p) the captured step goes on
    to draw `u` = torch.rand(B) (fresh numbers per replay: the capture
    registers the default generator) and to sample the next id from
    `logits` into `ids` with ops.sample_logits. After a replay `ids` is the
    next step's input already and `step()` takes no argument."""

    def __init__(self, model, cache, sample_key: str, prediction_key: str,
                 sampler: Optional[tuple] = None):
        self.cache = cache
        self.sample_key = sample_key
        self.sampler = sampler
        dev = cache.pos_dev.device
        B = cache.pos_dev.shape[0]
        self.ids = torch.zeros(B, 1, dtype=torch.long, device=dev)
        pos = cache.pos
        if pos + 1 > cache.max_len:
            raise ValueError("KV cache is full: nothing left to decode")

        def rewind():
            cache.pos = pos
            cache.pos_dev.fill_(pos)

        def one_step():
            logits = model.forward_cached({sample_key: self.ids},
                                          cache)[prediction_key]
            if sampler is not None:
                from modalities_amd.ops import sample_logits
                self.u = torch.rand(B, device=dev)
                sample_logits(logits[:, -1], self.u, self.ids, *sampler)
            return logits

        try:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                one_step()
            torch.cuda.current_stream(dev).wait_stream(side)
            rewind()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.logits = one_step()
        finally:
            rewind()

    def step(self, next_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decode one token per row; returns the static logits [B, 1, V].
        `next_ids` None (a graph with a sampler, from its second step on)
        decodes the ids the last replay sampled."""
        if self.cache.pos + 1 > self.cache.max_len:
            raise ValueError(f"KV cache overflow: {self.cache.pos}+1 > "
                             f"{self.cache.max_len}")
        if next_ids is not None:
            self.ids.copy_(next_ids)
        elif self.sampler is None:
            raise ValueError("DecodeGraph.step: a graph without a sampler "
                             "needs next_ids")
        self.graph.replay()
        self.cache.pos += 1
        return self.logits


def capture_decode_graph(model, cache, sample_key: str = "input_ids",
                         prediction_key: str = "logits",
                         sampler: Optional[tuple] = None
                         ) -> Optional[DecodeGraph]:
    """A DecodeGraph when the model decodes on the GPU through the decode
    kernels and the capture succeeds; None (decode eagerly) otherwise."""
    route = getattr(model, "_decode_route", None)
    if route is None or not cache.pos_dev.is_cuda \
            or not route(cache.pos_dev):
        return None
    try:
        if sampler is None:
            return DecodeGraph(model, cache, sample_key, prediction_key)
        return DecodeGraph(model, cache, sample_key, prediction_key, sampler)
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
                 decode_weight_format: Optional[str] = None,
                 kv_cache_format: Optional[str] = None,
                 device_sampling: bool = False,
                 prefill_chunk_tokens: Optional[int] = None):
        if decode_weight_format is not None \
                and not hasattr(model, "prepare_decode_weights"):
            raise ValueError(
                f"decode_weight_format={decode_weight_format!r}: "
                f"{type(model).__name__} has no prepare_decode_weights")
        if kv_cache_format is not None:
            from modalities_amd.ops.attention import KV_CACHE_FORMATS
            if kv_cache_format not in KV_CACHE_FORMATS:
                raise ValueError(f"kv_cache_format must be None or one of "
                                 f"{KV_CACHE_FORMATS}, got "
                                 f"{kv_cache_format!r}")
            if not hasattr(model, "new_kv_cache"):
                raise ValueError(
                    f"kv_cache_format={kv_cache_format!r}: "
                    f"{type(model).__name__} has no KV cache")
        if prefill_chunk_tokens is not None and (
                not isinstance(prefill_chunk_tokens, int)
                or isinstance(prefill_chunk_tokens, bool)
                or prefill_chunk_tokens < 2):
            raise ValueError(f"prefill_chunk_tokens must be None or an "
                             f"integer >= 2, got {prefill_chunk_tokens!r}")
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
        self.kv_cache_format = kv_cache_format
        self.device_sampling = device_sampling
        self.prefill_chunk_tokens = prefill_chunk_tokens

    def _prefill(self, input_ids: torch.Tensor, cache) -> dict:
        """The prompt into the cache: in one piece, or in chunks of
        prefill_chunk_tokens with the multi-token decode route open to
        them. Returns the output of the last piece."""
        n = self.prefill_chunk_tokens
        if n is None or input_ids.shape[1] <= n:
            return self.model.forward_cached({self.sample_key: input_ids},
                                             cache)
        from modalities_amd.ops.attention import (decode_chunk_tokens,
                                                  set_decode_chunk_tokens)
        was = decode_chunk_tokens()
        set_decode_chunk_tokens(max(was, n))
        try:
            for p in range(0, input_ids.shape[1], n):
                out = self.model.forward_cached(
                    {self.sample_key: input_ids[:, p:p + n]}, cache)
        finally:
            set_decode_chunk_tokens(was)
        return out

    def _sampler(self) -> tuple:
        """(temperature, top_k, top_p) as ops.sample_logits takes them."""
        return (float(self.temperature), int(self.top_k or 0),
                float(self.top_p or 0.0))

    def _sample(self, logits: torch.Tensor) -> torch.Tensor:
        """Greedy (temperature==0) or temperature sampling with optional
        top-k / nucleus (top-p) filtering. With device_sampling: the same
        through ops.sample_logits, on the logits as they are stored."""
        if self.device_sampling:
            from modalities_amd.ops import sample_logits
            B = logits.shape[0]
            u = torch.rand(B, device=logits.device)
            ids = torch.empty(B, 1, dtype=torch.long, device=logits.device)
            return sample_logits(logits, u, ids, *self._sampler())
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
            kw = {} if self.kv_cache_format is None \
                else {"kv_format": self.kv_cache_format}
            cache = self.model.new_kv_cache(input_ids.shape[0],
                                            max_len=self.sequence_length,
                                            **kw)
            out = self._prefill(input_ids, cache)
        else:
            out = self.model({self.sample_key: input_ids})

        graph = None
        graph_tried = not (self.use_decode_graph and cache is not None)
        next_id = None   # set where a graph replay sampled it on the device
        for i in range(max_new):
            if next_id is None:
                logits = out[self.prediction_key][:, -1, :]
                next_id = self._sample(logits if self.device_sampling
                                       else logits.float())
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
                        self.prediction_key,
                        self._sampler() if self.device_sampling else None)
                if graph is not None and graph.sampler is not None:
                    out = {self.prediction_key: graph.step(
                        None if next_id is graph.ids else next_id)}
                    next_id = graph.ids
                    continue
                if graph is not None:
                    out = {self.prediction_key: graph.step(next_id)}
                else:
                    out = self.model.forward_cached(
                        {self.sample_key: next_id}, cache)
            else:
                input_ids = torch.cat([input_ids, next_id], dim=1)
                out = self.model({self.sample_key: input_ids})
            next_id = None
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
