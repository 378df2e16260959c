"""Engine-backed stand-in for the reference's `OmChatQwen25VLForCausalLM`
(vlm_fo1/model/language_model/omchat_qwen2_5_vl.py:28-572): exposes what the reference's callers touch —
`generate(**prepare_inputs(...))`, `config` attribute access, `get_vision_tower()/get_vision_tower_aux()`,
`eval()/to()` — and owns generation itself (greedy loop + KV cache in the engine) instead of leaning on HF
`GenerationMixin` internals, which drifted under transformers 5."""
from __future__ import annotations

import types
from typing import Dict, List, Optional

import torch

from vlm_fo1_amd.davit import DAVIT_LARGE
from vlm_fo1_amd.llm import LLMConfig
from vlm_fo1_amd.model import FO1Config, FO1Engine
from vlm_fo1_amd.vit import ViTConfig


class FO1HFConfig:
    """`config.json` with attribute access (`getattr(config, 'mm_*', default)` as the reference reads it:
    omchat_arch.py:11-31, builder.py:65-70, mm_utils.py:593)."""

    def __init__(self, d: dict, generation: Optional[dict] = None):
        self._d = dict(d)
        self._gen = dict(generation or {})
        for k, v in d.items():
            if k == "vision_config" and isinstance(v, dict):
                v = types.SimpleNamespace(**v)
            setattr(self, k, v)

    def to_dict(self):
        return dict(self._d)

    # ---- engine configuration derived from the checkpoint's config (asserted, never guessed) ----
    def engine_config(self) -> FO1Config:
        d = self._d
        txt = d.get("text_config", d)
        vis = d["vision_config"]
        rs = txt.get("rope_scaling") or d.get("rope_scaling") or {}
        heads = txt["num_attention_heads"]
        llm = LLMConfig(hidden_size=txt["hidden_size"], num_layers=txt["num_hidden_layers"], num_heads=heads,
                        num_kv_heads=txt["num_key_value_heads"], head_dim=txt["hidden_size"] // heads,
                        intermediate_size=txt["intermediate_size"], vocab_size=txt["vocab_size"],
                        rms_norm_eps=txt.get("rms_norm_eps", 1e-6), rope_theta=txt.get("rope_theta", 1e6),
                        mrope_section=tuple(rs.get("mrope_section", (16, 24, 24))),
                        max_seq=min(int(d.get("tokenizer_model_max_length") or 8192), 32768))
        vit = ViTConfig(depth=vis["depth"], hidden_size=vis["hidden_size"], num_heads=vis["num_heads"],
                        intermediate_size=vis["intermediate_size"], out_hidden_size=vis["out_hidden_size"],
                        patch_size=vis.get("patch_size", 14), spatial_merge_size=vis.get("spatial_merge_size", 2),
                        temporal_patch_size=vis.get("temporal_patch_size", 2), in_channels=vis.get("in_channels", vis.get("in_chans", 3)),
                        window_size=vis.get("window_size", 112), fullatt_block_indexes=tuple(vis.get("fullatt_block_indexes", (7, 15, 23, 31))))
        unsupported = []
        use_vt = bool(d.get("mm_use_vision_tower_region_feature", False))       # reference default: omchat_arch.py:23
        if not use_vt:
            # The reference itself cannot run this value: HFREModule.__call__ never binds `out_box_feat` without the vt branch and
            # raises UnboundLocalError (hybrid_finegrained_region_encoder.py:456/469; pinned by tests/test_oracle_hfre.py).  The
            # engine's aux-only route is the evident reading (aux block + aux-box embedding) — loadable, labelled as an extension.
            import warnings
            warnings.warn("mm_use_vision_tower_region_feature=False: the reference's HFRE raises UnboundLocalError for this configuration; "
                          "the engine runs its aux-only extension (aux region block + box embedding from the aux boxes)", stacklevel=2)
            if d.get("mm_use_vt_region_feature_only", False):
                unsupported.append("mm_use_vt_region_feature_only without mm_use_vision_tower_region_feature")
        if d.get("mm_region_feature_combination", "concat") not in ("concat", "concat_aux_pos"):
            unsupported.append(f"mm_region_feature_combination={d.get('mm_region_feature_combination')!r}")
        if d.get("mm_pos_embedding_strategy", "bbox_based") not in ("bbox_based", "feature_map_based", "hybrid"):
            unsupported.append(f"mm_pos_embedding_strategy={d.get('mm_pos_embedding_strategy')!r}")
        aux = str(d.get("mm_vision_tower_aux", "davit-large"))
        if "davit-large" not in aux:
            unsupported.append(f"mm_vision_tower_aux={aux!r}")
        if unsupported:
            raise NotImplementedError("checkpoint configuration not built for the MI355X engine: " + ", ".join(unsupported))
        return FO1Config(vit=vit, llm=llm, mm_projector_type=d.get("mm_projector_type", "linear"),
                         mm_projector_aux_type=d.get("mm_projector_aux_type", "linear"),
                         mm_use_simpleFPN_for_vt=bool(d.get("mm_use_simpleFPN_for_vt", False)),
                         mm_region_hidden_size=int(d["mm_region_hidden_size"]), mm_roi_output_size=int(d.get("mm_roi_output_size", 7)),
                         mm_apply_position_embedding=bool(d.get("mm_apply_position_embedding", True)),
                         mm_pos_embedding_strategy=d.get("mm_pos_embedding_strategy", "bbox_based"),
                         mm_apply_region_layer_norm=bool(d.get("mm_apply_region_layer_norm", False)),
                         mm_region_feature_combination=d.get("mm_region_feature_combination", "concat"),
                         mm_use_vt_region_feature_only=bool(d.get("mm_use_vt_region_feature_only", False)),
                         mm_use_vision_tower_region_feature=use_vt)

    def eos_ids(self) -> List[int]:
        e = self._gen.get("eos_token_id", self._d.get("eos_token_id"))
        if e is None:
            return []
        return list(e) if isinstance(e, (list, tuple)) else [int(e)]


class GenerateLogprobsOutput:
    """What generate(output_logprobs=True) returns: .sequences = the tensor generate() returns otherwise ([1, L_in + new]), .logprobs float32
    [1, new], .top_ids int64 [1, new, n] and .top_logprobs float32 [1, new, n] with n = top_logprobs."""

    def __init__(self, sequences, logprobs, top_ids, top_logprobs):
        self.sequences, self.logprobs, self.top_ids, self.top_logprobs = sequences, logprobs, top_ids, top_logprobs


class _TowerHandle:
    """What callers get from `get_vision_tower()` / `get_vision_tower_aux()`: loaded flag, config, processor."""

    def __init__(self, config, image_processor=None):
        self.is_loaded = True
        self.config = config
        self.image_processor = image_processor


class FO1ForCausalLM:
    def __init__(self, config: FO1HFConfig, weights: Dict[str, Dict[str, torch.Tensor]], device="cuda"):
        self.config = config
        self.device = torch.device(device)
        self.dtype = torch.bfloat16
        self.engine = FO1Engine(config.engine_config(), weights, device)
        self._vt = _TowerHandle(getattr(config, "vision_config", None))
        self._vt_aux = _TowerHandle(types.SimpleNamespace(**DAVIT_LARGE))
        self.use_graph = True   # replay a captured hipGraph per input-shape signature

    @classmethod
    def from_engine(cls, config: FO1HFConfig, engine: FO1Engine) -> "FO1ForCausalLM":
        """The drop-in model object around an engine that already exists (bench.py's `driver_level` block measures the eval drivers'
        own loop on the engine whose passes it has just timed, instead of loading a second copy of the weights)."""
        m = cls.__new__(cls)
        m.config, m.device, m.dtype, m.engine = config, torch.device(engine.dev), torch.bfloat16, engine
        m._vt = _TowerHandle(getattr(config, "vision_config", None))
        m._vt_aux = _TowerHandle(types.SimpleNamespace(**DAVIT_LARGE))
        m.use_graph = True
        return m

    def replica(self) -> "FO1ForCausalLM":
        """Same weights, private per-request state (KV cache, graphs, scratch): one per worker thread / HIP stream, so several
        requests can be in flight on one GPU (vlm_fo1_amd.sharded_eval.run_sharded with a list of workers)."""
        import copy
        r = copy.copy(self)
        r.engine = self.engine.replica()
        r.__dict__.pop("_worker_replicas", None)       # (sharded_eval.request_workers keeps the model's replicas on the model)
        return r

    # ---- nn.Module-ish surface the reference drivers call ----
    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def get_model(self):
        return self

    def get_vision_tower(self):
        return self._vt

    def get_vision_tower_aux(self):
        return self._vt_aux

    # ---- generation ----
    def _request(self, inputs, images, images_aux, image_grid_thws, bbox_list):
        """One prepare_inputs(...) kwargs set -> the engine's request dict."""
        if inputs is None or inputs.dim() != 2 or inputs.shape[0] != 1:
            raise ValueError("generate: `inputs` must be a [1, L] id tensor (the reference drivers are batch-1)")
        if not images or image_grid_thws is None:
            raise ValueError("generate: the engine path needs one image (images / image_grid_thws)")
        dev = self.device
        grid = image_grid_thws[0].reshape(-1, 3)[0].tolist()
        if grid[0] != 1:
            raise NotImplementedError("video grids (t > 1) are outside the hot path")
        if not images_aux:
            raise ValueError("generate: images_aux is required (mm_use_region_index_token checkpoints)")
        boxes = None
        if bbox_list is not None and len(bbox_list) > 0 and bbox_list[0] is not None:
            boxes = bbox_list[0].to(device=dev, dtype=torch.float32)
        ids = getattr(inputs, "_fo1_ids", None)      # prepare_inputs keeps the host list next to the device tensor
        if ids is None or len(ids) != inputs.shape[1]:
            ids = inputs[0].tolist()
        self._check_model_max_length(ids, (grid[1] // 2) * (grid[2] // 2))
        return dict(ids=ids, pix=images[0].to(device=dev, dtype=torch.bfloat16), grid=(grid[1], grid[2]),
                    aux=images_aux[0].to(device=dev, dtype=torch.bfloat16), boxes=boxes)

    def _check_model_max_length(self, ids, n_image_tokens: int) -> None:
        """`tokenizer_model_max_length` semantics of the reference splice (omchat_qwen2_5_vl.py:374-378): the spliced embeddings and
        labels are cut to that length but `new_input_ids` is NOT, so with the default right padding the very next statement
        (`new_input_ids_padded[i, :cur_len] = cur_new_input_ids`, :411) fails with torch's size-mismatch RuntimeError — an over-long
        prompt never reaches the LLM.  Same here: same exception type, same sizes in the message.  (Left padding would run the
        reference on all-BOS ids with text-only positions; that variant is not built.)"""
        limit = getattr(self.config, "tokenizer_model_max_length", None)
        if limit is None:
            return
        from vlm_fo1_amd.llm import IMAGE_TOKEN_INDEX
        spliced = len(ids) + sum(n_image_tokens - 1 for t in ids if t == IMAGE_TOKEN_INDEX)      # a <regionfeat> sentinel becomes one row
        if spliced <= int(limit):
            return
        if getattr(self.config, "tokenizer_padding_side", "right") == "left":
            raise NotImplementedError("prompt longer than tokenizer_model_max_length with left padding is not built")
        raise RuntimeError(f"The expanded size of the tensor ({int(limit)}) must match the existing size ({spliced}) at non-singleton dimension 0.  "
                           f"Target sizes: [{int(limit)}].  Tensor sizes: [{spliced}]  (spliced prompt exceeds tokenizer_model_max_length; the "
                           "reference fails at omchat_qwen2_5_vl.py:411 in the same way)")

    def _device_stop_ids(self, stopping_criteria) -> Optional[List[int]]:
        """EOS ids + the ids of single-token stop keywords (mm_utils.KeywordsStoppingCriteria with `<|im_end|>`): the stop rule the
        batched decoder evaluates on the device.  None when a criterion cannot be expressed as 'last token in a set'."""
        ids = list(self.config.eos_ids())
        for c in (stopping_criteria or []):
            kws = getattr(c, "keyword_ids", None)
            if kws is None or any(int(k.numel()) != 1 for k in kws):
                return None
            ids += [int(k.reshape(-1)[0]) for k in kws]
        ids = sorted(set(ids))
        from vlm_fo1_amd.llm import BatchDecoder
        return ids if len(ids) <= BatchDecoder.MAX_STOP else None     # more ids than the device rule holds: host loop, nothing dropped

    @staticmethod
    def _fits_device_loop(max_new_tokens) -> bool:
        from vlm_fo1_amd.llm import BatchDecoder
        return int(max_new_tokens) <= BatchDecoder.IDS_CAP

    @staticmethod
    def _sampling_plan(kwargs: dict, generation_config: Optional[dict] = None) -> Optional[dict]:
        """generate()'s sampling arguments -> None (greedy) or dict(temperature, top_p, top_k, seed) for the device sampler.  Sampling is on
        iff do_sample, as in HF generate: do_sample=False with a temperature decodes greedily.  top_k defaults to the checkpoint's
        generation_config.json, else 50 (HF's default); seed is the `seed` kwarg, else 63 bits drawn from torch's default CPU generator at
        call time — torch.manual_seed makes a run reproducible, as under HF.  The generator itself is Philox, not torch's: the ids are not
        HF's ids, the distribution is."""
        if not kwargs.get("do_sample"):
            return None
        import math
        gen = generation_config or {}
        t = kwargs.get("temperature")
        try:      # any real scalar HF accepts (Python and numpy numbers, 0-d tensors); a bool is not a temperature
            tv = None if t is None or isinstance(t, bool) else float(t)
        except (TypeError, ValueError):
            tv = None
        # (the device holds it as fp32 and multiplies by its reciprocal: both must be positive finite numbers there)
        t32 = None if tv is None else torch.tensor(tv, dtype=torch.float32)
        if tv is None or not (tv > 0 and math.isfinite(float(t32)) and math.isfinite(float(t32.reciprocal()))):
            raise ValueError(f"do_sample=True needs a positive finite temperature (got {t!r})")
        top_p = kwargs.get("top_p")
        top_p = 1.0 if top_p is None else float(top_p)
        if not 0.0 < top_p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1] (got {top_p!r})")
        top_k = kwargs.get("top_k")
        if top_k is None:
            top_k = gen.get("top_k")
        top_k = 50 if top_k is None else int(top_k)
        if top_k < 0:
            raise ValueError(f"top_k must be >= 0, 0 switches it off (got {top_k!r})")
        seed = kwargs.get("seed")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        return dict(temperature=tv, top_p=top_p, top_k=top_k, seed=int(seed) & (2 ** 64 - 1))

    @staticmethod
    def _penalty_plan(kwargs: dict) -> Optional[float]:
        """generate()'s repetition_penalty -> None (off: None or 1.0) or the value.  Off unless the caller passes one, whatever the
        checkpoint's generation_config.json says: nothing that decodes without the argument may change."""
        import math
        p = kwargs.get("repetition_penalty")
        if p is None:
            return None
        try:
            pv = None if isinstance(p, bool) else float(p)
        except (TypeError, ValueError):
            pv = None
        p32 = None if pv is None else float(torch.tensor(pv, dtype=torch.float32))      # (the device holds it as fp32)
        if pv is None or not (math.isfinite(p32) and p32 > 0):
            raise ValueError(f"repetition_penalty must be a positive finite number, 1.0 switches it off (got {p!r})")
        return None if p32 == 1.0 else pv

    @staticmethod
    def _rule_plan(kwargs: dict, eos_ids=()) -> Optional[dict]:
        """generate()'s suppress_tokens / begin_suppress_tokens / bad_words_ids / min_new_tokens / allowed_token_ids -> None (all off, the
        default, whatever generation_config.json holds) or the engine's token-rule keys (vlm_fo1_amd.llm.token_rule, which checks the ids
        against the vocabulary): ban = suppress_tokens + the single-token bad words (a longer entry is a NotImplementedError naming it),
        ban_first = begin_suppress_tokens, allow = allowed_token_ids, ban_until = (min_new_tokens, the EOS ids) — HF's
        MinNewTokensLengthLogitsProcessor: the EOS ids, not the stop keywords.  The values are sorted tuples: equal rules compare equal."""
        def ids(name):
            v = kwargs.get(name)
            if v is None:
                return None
            if isinstance(v, torch.Tensor):
                v = v.reshape(-1).tolist()
            if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
                raise ValueError(f"{name}: a list of token ids (got {v!r})")
            return list(v)
        plan = {}
        ban = list(ids("suppress_tokens") or [])
        words = kwargs.get("bad_words_ids")
        if words is not None:
            for w in words:
                w = w.reshape(-1).tolist() if isinstance(w, torch.Tensor) else list(w)
                if len(w) != 1:
                    raise NotImplementedError(f"bad_words_ids: only single-token entries are banned on the device (got {w!r})")
                ban.append(w[0])
        if ban:
            plan["ban"] = ban
        if ids("begin_suppress_tokens"):
            plan["ban_first"] = ids("begin_suppress_tokens")
        if ids("allowed_token_ids") is not None:
            plan["allow"] = ids("allowed_token_ids")      # (an empty allow-list is the engine's ValueError)
        n = kwargs.get("min_new_tokens")
        if n is not None:
            if isinstance(n, bool) or not isinstance(n, int) or n < 0:
                raise ValueError(f"min_new_tokens must be an integer >= 0 (got {n!r})")
            if n > 0 and len(tuple(eos_ids)):
                plan["ban_until"] = (n, tuple(sorted(int(t) for t in eos_ids)))
        for k in ("ban", "ban_first", "allow"):
            if k in plan:
                if any(isinstance(t, (bool, float)) or not hasattr(t, "__index__") for t in plan[k]):
                    raise ValueError(f"{k}: token ids are integers (got {plan[k]!r})")
                plan[k] = tuple(sorted(set(int(t) for t in plan[k])))
        return plan or None

    @staticmethod
    def _steer_plan(kwargs: dict) -> Optional[dict]:
        """generate()'s logit_bias / sequence_bias / frequency_penalty / presence_penalty -> None (all off, the default, whatever
        generation_config.json holds) or the engine's steer keys (vlm_fo1_amd.llm.token_steer, which checks the ids against the vocabulary
        and rounds the values to bf16): bias = {id: value} from logit_bias ({id: value}; an id may be an integer or its decimal string, as
        OpenAI-shaped callers send it) and sequence_bias (HF's forms {(id,): value} or [[[id], value], ...]; an entry longer than one token is
        a NotImplementedError naming it), the two summed per id; an id whose sum is 0 has no bias.  frequency_penalty / presence_penalty: any
        finite fp32 value, 0 or None = off.  ValueError: a value that is a bool, not a number or not finite."""
        import math

        def number(v, what):
            if isinstance(v, bool):
                raise ValueError(f"{what}: a finite number (got {v!r})")
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"{what}: a finite number (got {v!r})") from None
            if not math.isfinite(f) or not math.isfinite(float(torch.tensor(f, dtype=torch.float32))):
                raise ValueError(f"{what}: a finite number (got {v!r}); to forbid a token use suppress_tokens, to force a set allowed_token_ids")
            return f

        def token(t, what):
            if isinstance(t, str) and t.strip().lstrip("-").isdigit():
                t = int(t)
            if isinstance(t, torch.Tensor) and t.numel() == 1 and not t.is_floating_point():
                t = int(t.item())
            if isinstance(t, (bool, float)) or not hasattr(t, "__index__"):
                raise ValueError(f"{what}: token ids are integers (got {t!r})")
            return int(t)

        bias: Dict[int, float] = {}
        lb = kwargs.get("logit_bias")
        if lb is not None:
            if not hasattr(lb, "items"):
                raise ValueError(f"logit_bias: a dict {{token id: value}} (got {type(lb).__name__})")
            for t, v in lb.items():
                t = token(t, "logit_bias")
                bias[t] = bias.get(t, 0.0) + number(v, f"logit_bias[{t}]")
        sb = kwargs.get("sequence_bias")
        if sb is not None:
            if isinstance(sb, (str, bytes)) or not (hasattr(sb, "items") or hasattr(sb, "__iter__")):
                raise ValueError(f"sequence_bias: {{(id,): value}} or [[[id], value], ...] (got {sb!r})")
            entries = list(sb.items()) if hasattr(sb, "items") else [tuple(e) for e in sb]
            for e in entries:
                if len(e) != 2:
                    raise ValueError(f"sequence_bias: an entry is (token sequence, value) (got {e!r})")
                seq, v = e
                seq = seq.reshape(-1).tolist() if isinstance(seq, torch.Tensor) else (list(seq) if hasattr(seq, "__iter__") and not isinstance(seq, (str, bytes)) else [seq])
                if len(seq) != 1:
                    raise NotImplementedError(f"sequence_bias: only single-token entries are biased on the device (got {seq!r})")
                t = token(seq[0], "sequence_bias")
                bias[t] = bias.get(t, 0.0) + number(v, f"sequence_bias[{t}]")
        plan = {}
        bias = {t: number(v, f"the summed bias of token {t}") for t, v in sorted(bias.items()) if v != 0}
        if bias:
            plan["bias"] = bias
        for name in ("frequency_penalty", "presence_penalty"):
            v = kwargs.get(name)
            if v is not None and number(v, name) != 0:
                plan[name] = number(v, name)
        return plan or None

    @classmethod
    def _decode_plan(cls, kwargs: dict, generation_config: Optional[dict] = None, eos_ids=()) -> Optional[dict]:
        """_sampling_plan, _penalty_plan, _rule_plan and _steer_plan as the one dict the engine takes per request: None = plain greedy; a
        sampled request's dict gains repetition_penalty, the token-rule keys and the steer keys; a greedy request with a penalty, a rule or a
        steer is dict(greedy=True, ...).  guide (a vlm_fo1_amd.guide.TokenGuide, or None = off; anything else is a ValueError) rides in the
        dict as the engine's `guide` key."""
        sampling, pen, rule = cls._sampling_plan(kwargs, generation_config), cls._penalty_plan(kwargs), cls._rule_plan(kwargs, eos_ids)
        guide, steer = cls._guide_plan(kwargs), cls._steer_plan(kwargs)
        if pen is None and rule is None and guide is None and steer is None:
            return sampling
        plan = dict(greedy=True) if sampling is None else dict(sampling)
        if pen is not None:
            plan["repetition_penalty"] = pen
        plan.update(rule or {})
        plan.update(steer or {})
        if guide is not None:
            plan["guide"] = guide
        return plan

    @staticmethod
    def _guide_plan(kwargs: dict):
        guide = kwargs.get("guide")
        if guide is None:
            return None
        from vlm_fo1_amd.guide import TokenGuide
        if not isinstance(guide, TokenGuide):
            raise ValueError(f"guide: a vlm_fo1_amd.guide.TokenGuide, as region_guide() builds one (got {type(guide).__name__})")
        return guide

    def region_guide(self, tokenizer, n_regions: int, close: bool = False):
        """The guide of the FO1 answer language `<ground>label</ground><objects><region3>...</objects>` for a request with n_regions boxes
        (vlm_fo1_amd.guide.region_answer): the five structural ids and the <regionK> ids from tokenizer.convert_tokens_to_ids — every
        <regionK> the tokenizer knows, K = 0, 1, ... —, the stop ids from config.eos_ids().  ValueError: a token that is not a single id of
        the vocabulary, or fewer <regionK> tokens than n_regions.
        close=True: the answer also closes its structure before max_new_tokens runs out — generate(guide=, max_new_tokens=k) ends outside
        `<ground>` / `<objects>` for every k; the budget is generate()'s max_new_tokens, no further keyword."""
        from vlm_fo1_amd.guide import region_answer
        V = self.engine.cfg.llm.vocab_size
        unk = getattr(tokenizer, "unk_token_id", None)

        def one(tok):
            t = tokenizer.convert_tokens_to_ids(tok)
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < V or (unk is not None and t == unk):
                return None
            return t
        struct = [one(t) for t in ("<ground>", "</ground>", "<objects>", "</objects>")]
        if any(t is None for t in struct):
            raise ValueError("region_guide: <ground>, </ground>, <objects> and </objects> must each be a single id of the vocabulary")
        regions = []
        while one(f"<region{len(regions)}>") is not None:
            regions.append(one(f"<region{len(regions)}>"))
        if int(n_regions) > len(regions):
            raise ValueError(f"region_guide: the tokenizer has {len(regions)} <regionK> tokens, the request {int(n_regions)} boxes")
        return region_answer(V, *struct, regions, int(n_regions), self.config.eos_ids(), close=bool(close))

    @staticmethod
    def _logprob_plan(kwargs: dict) -> Optional[int]:
        """generate()'s output_logprobs / top_logprobs -> None (off, the default) or the top-n (0 .. 8) of the record the engine keeps."""
        on = bool(kwargs.get("output_logprobs", False))
        n = kwargs.get("top_logprobs", 0)
        n = 0 if n is None else n
        from vlm_fo1_amd.ops import LOGPROB_TOP_MAX
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= LOGPROB_TOP_MAX:
            raise ValueError(f"top_logprobs must be an integer in 0..{LOGPROB_TOP_MAX} (got {n!r})")
        if n and not on:
            raise ValueError("top_logprobs needs output_logprobs=True")
        return n if on else None

    @staticmethod
    def _with_logprobs(sequences: torch.Tensor, rec) -> "GenerateLogprobsOutput":
        dev = sequences.device
        return GenerateLogprobsOutput(sequences=sequences, logprobs=rec.logprob.unsqueeze(0).to(dev),
                                      top_ids=rec.top_ids.to(torch.int64).unsqueeze(0).to(dev), top_logprobs=rec.top_logprobs.unsqueeze(0).to(dev))

    def _batch_plan(self, requests_kwargs: List[dict]):
        """Validation shared by generate_many / generate_many_async -> (engine requests, max_new_tokens, device stop ids, sampling), or None
        when the batch must take the one-by-one host loop (a stop criterion the device rule cannot express, a budget beyond its id buffer).
        Requests may differ in output_logprobs / top_logprobs, pool or not (they are checked here; the callers read them per request).
        sampling: None, the batch's one dict, or — with the decode pool enabled, whose slots each carry their own parameters — a list with
        one dict or None per request when the requests differ (request i draws on stream i of its own seed)."""
        k0 = requests_kwargs[0]
        gen = getattr(self.config, "_gen", None)
        for kw in requests_kwargs:
            self._logprob_plan(kw)
        stop = self._device_stop_ids(k0.get("stopping_criteria"))
        if stop is None or not self._fits_device_loop(k0.get("max_new_tokens", 512)):
            return None
        pooled = getattr(getattr(self, "engine", None), "_pool_svc", None) is not None
        eos = tuple(self.config.eos_ids())

        def values(kw):      # what a packed batch without the pool must share
            sp = self._sampling_plan(dict(kw, seed=0), gen)
            rule = self._rule_plan(kw, eos)
            return ((None if sp is None else (sp["temperature"], sp["top_p"], sp["top_k"])), self._penalty_plan(kw), rule and tuple(sorted(rule.items())),
                    self._guide_plan(kw), self._steer_plan(kw))
        v0 = values(k0)
        mixed = False
        for kw in requests_kwargs[1:]:       # one budget and one stop rule per packed batch: refuse a mixed batch rather than apply the first's
            if int(kw.get("max_new_tokens", 512)) != int(k0.get("max_new_tokens", 512)) or \
                    self._device_stop_ids(kw.get("stopping_criteria")) != stop:
                raise ValueError("generate_many: every request of a batch must share max_new_tokens and stopping criteria")
            v = values(kw)
            if v != v0 or (v[0] is not None and kw.get("seed") != k0.get("seed")):
                mixed = True
                if pooled:
                    continue
                if v != v0:      # without the pool one BatchDecoder group decodes the batch with one sampling
                    raise ValueError("generate_many: every request of a batch must share do_sample, temperature, top_p and top_k "
                                     "(and repetition_penalty, the token-rule keywords, the guide and the steering keywords) unless the decode pool is enabled")
                raise ValueError("generate_many: every request of a sampled batch must share seed (request i draws on stream i of the one seed)")
        sampling = [self._decode_plan(kw, gen, eos) for kw in requests_kwargs] if mixed else self._decode_plan(k0, gen, eos)
        reqs = [self._request(kw.get("inputs"), kw.get("images"), kw.get("images_aux"), kw.get("image_grid_thws"), kw.get("bbox_list"))
                for kw in requests_kwargs]
        return reqs, int(k0.get("max_new_tokens", 512)), stop, sampling

    @staticmethod
    def _assemble(requests_kwargs, reqs, new, recs=None) -> list:
        out = []
        for i, (kw, req, ids) in enumerate(zip(requests_kwargs, reqs, new)):
            inp = kw["inputs"]
            # [1, L_in + new] on the inputs' device, like HF generate — assembled on the host from the id lists both sides already hold
            # (one upload per request instead of an upload, a device concat and a read back)
            seq = torch.tensor([list(req["ids"]) + list(ids)], dtype=inp.dtype).to(inp.device)
            rec = None if recs is None else recs[i]
            out.append(seq if rec is None else FO1ForCausalLM._with_logprobs(seq, rec))      # (a request with output_logprobs: the object generate() returns)
        return out

    @torch.no_grad()
    def generate_many(self, requests_kwargs: List[dict]) -> List[torch.LongTensor]:
        """Greedy generation for several prepare_inputs(...) kwargs sets at once: the images go through ONE packed prefill pass and
        the sequences decode together (weights streamed once per step, stop rule on the device).  Each result is [1, L_in + new]
        exactly as generate() returns it.  max_new_tokens / stopping criteria are taken from the first request (the eval drivers use
        the same for every item).  With do_sample=True the batch shares temperature, top_p, top_k and seed (drawn from torch's generator
        once when none is given), and request i draws on stream i of that seed — also when the batch has to be decoded one by one."""
        if not requests_kwargs:
            return []
        plan = self._batch_plan(requests_kwargs)
        if plan is None:
            sampling = self._sampling_plan(requests_kwargs[0], getattr(self.config, "_gen", None))
            if sampling is None:
                return [self.generate(**kw) for kw in requests_kwargs]
            return [self.generate(**dict(kw, seed=sampling["seed"]), _stream=i) for i, kw in enumerate(requests_kwargs)]
        reqs, max_new, stop, sampling = plan
        lps = [self._logprob_plan(kw) for kw in requests_kwargs]
        if all(n is None for n in lps):
            new = self.engine.generate_batch(reqs, max_new_tokens=max_new, stop_ids=stop, use_graph=self.use_graph, sampling=sampling)
            return self._assemble(requests_kwargs, reqs, new)
        new, recs = self.engine.generate_batch(reqs, max_new_tokens=max_new, stop_ids=stop, use_graph=self.use_graph, sampling=sampling, logprobs=lps)
        return self._assemble(requests_kwargs, reqs, new, recs)

    @torch.no_grad()
    def generate_many_async(self, requests_kwargs: List[dict]):
        """generate_many in two halves for callers that keep several groups in flight (sharded_eval.run_sharded): the packed prefill
        runs now and its sequences join the engine's decode pool (FO1Engine.enable_decode_pool); the returned object's `result()` blocks
        until they have stopped and returns what generate_many returns.  Without a pool (or for a batch the device rule cannot take)
        the work is simply done now."""
        class _Ready:
            def __init__(self, value):
                self._value = value

            def result(self):
                return self._value

        if not requests_kwargs:
            return _Ready([])
        eng = self.engine
        plan = self._batch_plan(requests_kwargs) if getattr(eng, "_pool_svc", None) is not None else None
        if plan is None:
            return _Ready(self.generate_many(requests_kwargs))
        reqs, max_new, stop, sampling = plan      # (sampled and penalised requests join the pool too: every slot has its own parameters)
        lps = [self._logprob_plan(kw) for kw in requests_kwargs]
        handles, base = [], 0
        for grp in eng.split_passes(reqs):        # <= 32 requests and <= 64k ViT rows per pass
            part = sampling if sampling is None or isinstance(sampling, dict) else sampling[base:base + len(grp)]
            lpart = lps[base:base + len(grp)]
            handles.append(eng.submit_batch(grp, max_new, stop, self.use_graph, sampling=part, stream_base=base,
                                            logprobs=None if all(n is None for n in lpart) else lpart))
            base += len(grp)
        model = self

        class _Pending:
            def result(self):
                new = [ids for h in handles for ids in h.result()]
                recs = [r for h in handles for r in h.logprobs()]
                return model._assemble(requests_kwargs, reqs, new, recs)

        return _Pending()

    def _generate_sampled_host_loop(self, req, inputs, sampling, n_max, streamer, stopping_criteria, stream=0, logprobs=None):
        """Sampled decoding with the tokens handed to the host one by one (a streamer, or stop criteria the device rule cannot express): a
        BatchDecoder of ONE sequence stepped token by token — the kernels of the device loop, so the same seed draws the same ids whether or
        not a streamer listens (the single-sequence step of QwenLLM runs other GEMV / attention kernels: its logits differ in last bits, and
        a draw near an interval's end would then fall on the neighbouring token).  logprobs: the top-n of the log-probability record (None = off);
        a requesting generation takes this loop whatever its head, plain greedy as dict(greedy=True): the record launch belongs to the
        BatchDecoder's step, the single-sequence step of QwenLLM has none."""
        eng, dev = self.engine, self.device
        eng.prefill_batch([req], use_graph=self.use_graph)
        hp = eng._last_batch
        per = [dict(sampling, stream=stream)]      # (a greedy request with a repetition penalty takes this loop too: dict(greedy=True, ...))
        tok = eng._first_tokens(per, [req], n_max)      # (a closing guide's budget: the one dec.start() gets)
        dec = eng._decoder()
        lpa = {} if logprobs is None else dict(logprobs=logprobs, first_logprobs=eng._first_logprobs(logprobs, tok, 1))
        dec.start(hp["seqs"], hp["delta"], tok, n_max, (), sampling=per, prompt_ids=[req["ids"]], **lpa)
        eos = set(self.config.eos_ids())
        all_ids = inputs.to(dev)
        if streamer is not None:
            streamer.put(inputs.cpu())
        for i in range(n_max):
            t = tok.to(torch.long).reshape(1, 1)
            all_ids = torch.cat([all_ids, t.to(all_ids.dtype)], dim=1)
            if streamer is not None:
                streamer.put(t.cpu())
            stop_now = int(t.item()) in eos
            if not stop_now and stopping_criteria:
                stop_now = any(bool(c(all_ids, None)) for c in stopping_criteria)
            if stop_now or i + 1 == n_max:
                break
            dec.step(self.use_graph)
            tok = dec.plan[0, 1:2]          # the id the step accepted (its next embedding-gather entry)
        if streamer is not None:
            streamer.end()
        out = all_ids.to(inputs.device)
        return out if logprobs is None else self._with_logprobs(out, dec.logprobs()[0])

    @torch.no_grad()
    def generate(self, inputs=None, images=None, images_aux=None, image_grid_thws=None, bbox_list=None, do_sample=False,
                 temperature=0.0, max_new_tokens=512, streamer=None, top_p=1.0, use_cache=True, stopping_criteria=None,
                 pad_token_id=None, top_k=None, seed=None, repetition_penalty=None, _stream=0, output_logprobs=False, top_logprobs=0,
                 suppress_tokens=None, begin_suppress_tokens=None, bad_words_ids=None, min_new_tokens=None, allowed_token_ids=None, guide=None,
                 logit_bias=None, sequence_bias=None, frequency_penalty=None, presence_penalty=None, **unused):
        """Decoding of one prompt: greedy, or with do_sample=True temperature / top-k / top-p sampling on the device (_sampling_plan).
        Returns [1, L_in + new] like HF generate (the reference slices `output_ids[0, inputs.shape[1]:]`, inference.py:47-48).  Without a
        streamer and with id-set stop criteria the whole loop runs on the device (BatchDecoder, no per-token host read); otherwise tokens
        are handed to the host one by one — the picks are made on the device either way, and both loops draw the same ids.  A sampled
        generation records its ids in the BatchDecoder's buffer: max_new_tokens beyond BatchDecoder.IDS_CAP is a ValueError.  _stream: the
        Philox stream of the draws (generate_many's one-by-one loop passes the request's index).  repetition_penalty: None or 1.0 = off
        (the default, whatever generation_config.json holds); else HF's RepetitionPenaltyLogitsProcessor in front of the pick, over the
        prompt's and the generated ids, on the device; not finite or <= 0 is a ValueError.
        output_logprobs=True: returns a GenerateLogprobsOutput instead of the tensor — .sequences (that tensor), .logprobs float32 [1, new]
        (log-probability of every generated token under the model's own distribution: the log-softmax of the raw logits, before temperature,
        top-k / top-p and the penalty), .top_ids int64 / .top_logprobs float32 [1, new, top_logprobs] (the most likely tokens of each step,
        0 <= top_logprobs <= 8).  The records are kept in the BatchDecoder's buffers: max_new_tokens beyond IDS_CAP is a ValueError, and with
        a streamer or unexpressible stop criteria the generation steps a BatchDecoder of one (the same ids and records either way).
        suppress_tokens / bad_words_ids (single-token entries; a longer one is a NotImplementedError) / allowed_token_ids /
        begin_suppress_tokens / min_new_tokens: HF's processors of those names in front of the pick, on the device (_rule_plan; DESIGN.md
        section 14).  All default to off, whatever generation_config.json holds.  A constrained generation decodes as a penalised one does:
        in the BatchDecoder, stepped one by one with a streamer or unexpressible stop criteria; max_new_tokens beyond IDS_CAP is a ValueError.
        guide: None (off) or a vlm_fo1_amd.guide.TokenGuide — region_guide(tokenizer, n_regions) for the FO1 answer language, guide.ban_sequences
        for multi-token banned sequences: the banned set of every pick follows the guide's automaton state, which the head advances on the
        device; decoded as a constrained generation is.  max_new_tokens may still cut an answer short inside a structure unless the guide has
        accepting states (region_guide(..., close=True)): then the head closes the structure before the budget runs out.
        logit_bias={id: value} / sequence_bias (HF's forms, single-token entries; a longer one is a NotImplementedError): added to the token's
        logit in front of the repetition penalty, the two keywords summed per id; frequency_penalty / presence_penalty: the OpenAI count
        penalties over the generated tokens, subtracted after it (_steer_plan).  All default to off, whatever
        generation_config.json holds; a steered generation decodes as a penalised one does, max_new_tokens beyond IDS_CAP is a ValueError."""
        lpn = self._logprob_plan(dict(output_logprobs=output_logprobs, top_logprobs=top_logprobs))
        if lpn is not None and not self._fits_device_loop(max_new_tokens):
            from vlm_fo1_amd.llm import BatchDecoder
            raise ValueError(f"output_logprobs=True keeps at most {BatchDecoder.IDS_CAP} records per request (max_new_tokens={int(max_new_tokens)})")
        sampling = self._decode_plan(dict(do_sample=do_sample, temperature=temperature, top_p=top_p, top_k=top_k, seed=seed,
                                          repetition_penalty=repetition_penalty, suppress_tokens=suppress_tokens,
                                          begin_suppress_tokens=begin_suppress_tokens, bad_words_ids=bad_words_ids, min_new_tokens=min_new_tokens,
                                          allowed_token_ids=allowed_token_ids, guide=guide, logit_bias=logit_bias, sequence_bias=sequence_bias,
                                          frequency_penalty=frequency_penalty, presence_penalty=presence_penalty), getattr(self.config, "_gen", None),
                                     self.config.eos_ids())
        req = self._request(inputs, images, images_aux, image_grid_thws, bbox_list)
        dev = self.device
        stop = self._device_stop_ids(stopping_criteria) if streamer is None else None
        if sampling is not None and not self._fits_device_loop(max_new_tokens):
            from vlm_fo1_amd.llm import BatchDecoder
            raise ValueError(f"do_sample=True (and a repetition penalty or a token rule) draws at most {BatchDecoder.IDS_CAP} tokens per request (max_new_tokens={int(max_new_tokens)})")
        if stop is not None and (sampling is None or _stream == 0 or sampling.get("greedy")) and self._fits_device_loop(max_new_tokens):
            res = self.engine.generate_batch([req], max_new_tokens=int(max_new_tokens), stop_ids=stop, use_graph=self.use_graph, sampling=sampling,
                                             logprobs=lpn)
            ids = res[0] if lpn is None else res[0][0]
            seq = torch.cat([inputs.to(dev), torch.tensor([ids], dtype=inputs.dtype, device=dev)], dim=1).to(inputs.device)
            return seq if lpn is None else self._with_logprobs(seq, res[1][0])
        eng = self.engine
        if sampling is not None or lpn is not None:
            return self._generate_sampled_host_loop(req, inputs, sampling if sampling is not None else dict(greedy=True), int(max_new_tokens),
                                                    streamer, stopping_criteria, int(_stream), logprobs=lpn)
        out = eng.prefill(req["ids"], req["pix"], req["grid"], req["aux"], req["boxes"], use_graph=self.use_graph)
        eng.llm.reserve(eng.llm.kv_len + int(max_new_tokens))
        tok = out["next_token"]
        eos = set(self.config.eos_ids())
        all_ids = inputs.to(dev)
        if streamer is not None:
            streamer.put(inputs.cpu())
        first = True
        if self.use_graph:
            eng.llm.sync_decode_state()
        n_max = int(max_new_tokens)
        for i in range(n_max):
            t = tok.to(torch.long).reshape(1, 1)
            all_ids = torch.cat([all_ids, t.to(all_ids.dtype)], dim=1)
            if streamer is not None:
                streamer.put(t.cpu())
            tid = int(t.item())
            stop_now = tid in eos
            if not stop_now and stopping_criteria:
                stop_now = any(bool(c(all_ids, None)) for c in stopping_criteria)
            if stop_now or i + 1 == n_max:          # no decode step after the last token
                break
            if self.use_graph:
                _, tok = eng.llm.decode_step_graph(tok if first else None)
                first = False
            else:
                _, _, tok = eng.llm.decode_step(tok)
        if streamer is not None:
            streamer.end()
        return all_ids.to(inputs.device)
