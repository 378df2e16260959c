"""GPU test of the drop-in boundary end to end: a synthetic checkpoint directory (config.json + safetensors with
the reference's key names) -> vlm_fo1.model.builder.load_pretrained_model -> vlm_fo1.mm_utils.prepare_inputs ->
model.generate(**kwargs) -> slice / decode / extract exactly as the reference's inference.py:37-52 does."""
import json
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu


def noise_image(size, sigma, seed):
    """Grey Gaussian noise around 128 (what Image.effect_noise draws), from its own seeded generator: the pixels do not depend on what
    ran earlier in the process."""
    w, h = size
    g = np.random.default_rng(seed).normal(128.0, sigma, (h, w))
    return Image.fromarray(np.clip(np.rint(g), 0, 255).astype(np.uint8), "L")

CONFIG = {
    "model_type": "omchat_qwen2_5_vl", "hidden_size": 2048, "num_hidden_layers": 2, "num_attention_heads": 16,
    "num_key_value_heads": 2, "intermediate_size": 11008, "vocab_size": 8192, "rms_norm_eps": 1e-6, "rope_theta": 1000000.0,
    "rope_scaling": {"type": "mrope", "mrope_section": [16, 24, 24]}, "tie_word_embeddings": True, "eos_token_id": 151645,
    "vision_config": {"depth": 2, "hidden_size": 1280, "num_heads": 16, "intermediate_size": 3420, "out_hidden_size": 2048,
                      "patch_size": 14, "spatial_merge_size": 2, "temporal_patch_size": 2, "window_size": 112,
                      "fullatt_block_indexes": [1]},
    "mm_vision_tower": "qwen2.5-vl", "mm_vision_tower_aux": "davit-large", "mm_projector_type": "mlp2x_gelu",
    "mm_projector_aux_type": "mlp2x_gelu", "mm_use_vision_tower_region_feature": True, "mm_use_simpleFPN_for_vt": True,
    "mm_region_hidden_size": 5888, "mm_use_region_index_token": True, "aux_image_size": 768, "aux_image_aspect_ratio": "dynamic",
}


def checkpoint_state():
    from vlm_fo1.model.fo1_model import FO1HFConfig
    from vlm_fo1_amd.model import random_weights
    w = random_weights(FO1HFConfig(CONFIG).engine_config(), "cuda", seed=2)
    state = {}
    for k, v in w["vit"].items():
        state["model.vision_tower.image_tower." + k] = v
    for k, v in w["davit"].items():
        state["model.vision_tower_aux.image_tower." + k] = v
    for k, v in w["fpn"].items():
        state["model.object_vp_extractor.simple_fpn." + k] = v
    for k, v in w["proj"].items():
        state["model." + k] = v
    for k, v in w["llm"].items():
        state["model." + k] = v
    return state


def test_load_prepare_generate_roundtrip(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from test_dropin_surface import ToyTokenizer
    from vlm_fo1 import mm_utils as MU
    from vlm_fo1.model import builder
    from vlm_fo1.task_templates import OD_template
    model_dir = tmp_path / "VLM-FO1_Qwen2.5-VL-3B-v01"
    model_dir.mkdir()
    state = {k: v.cpu().contiguous() for k, v in checkpoint_state().items()}
    keys = sorted(state)
    half = len(keys) // 2                                   # sharded checkpoint: two safetensors files
    save_file({k: state[k] for k in keys[:half]}, str(model_dir / "model-00001-of-00002.safetensors"))
    save_file({k: state[k] for k in keys[half:]}, str(model_dir / "model-00002-of-00002.safetensors"))
    json.dump(CONFIG, open(model_dir / "config.json", "w"))
    json.dump({"eos_token_id": [151645, 151643]}, open(model_dir / "generation_config.json", "w"))

    class Tok(ToyTokenizer):
        def _enc(self, text):
            return [i % 8000 + 100 for i in super()._enc(text)]

        def decode(self, ids, **kw):
            return " ".join(str(int(i)) for i in ids)

    monkeypatch.setattr(builder, "_load_tokenizer", lambda p: Tok())
    # the synthetic checkpoint's embedding table has 8192 rows: move the hard-coded <|im_start|>/<|im_end|> ids
    # (151644/151645, mm_utils.py:481-482) inside it; with the real ids the engine must refuse instead of reading out of bounds
    monkeypatch.setattr(MU, "_IM_START_ID", 8190)
    monkeypatch.setattr(MU, "_IM_END_ID", 8191)
    tokenizer, model, procs = builder.load_pretrained_model(str(model_dir), device="cuda")
    assert model.config.mm_use_region_index_token is True and model.get_vision_tower().is_loaded

    img_path = str(tmp_path / "demo.jpg")
    noise_image((500, 399), 64, seed=1).convert("RGB").save(img_path)
    boxes = [[161.0, 11.0, 292.0, 127.0], [268.0, 61.0, 428.0, 226.0], [12.0, 100.0, 140.0, 227.0]]
    messages = [{"role": "user", "content": [{"type": "image_url", "image_url": {"url": img_path}},
                                             {"type": "text", "text": OD_template.format("orange")}], "bbox_list": boxes}]
    kw = MU.prepare_inputs(str(model_dir), model, procs, tokenizer, messages, max_tokens=5, top_p=0.05, temperature=0.0, do_sample=False)
    kw["streamer"] = None
    with torch.inference_mode():
        out = model.generate(**kw)
    L = kw["inputs"].shape[1]
    assert out.shape[0] == 1 and L < out.shape[1] <= L + 5 and torch.equal(out[0, :L].cpu(), kw["inputs"][0].cpu())
    new = out[0, L:].tolist()
    text = tokenizer.decode(out[0, L:]).strip()
    assert MU.extract_predictions_to_bboxes(text, boxes) == {}     # random weights: no markup, parser must cope
    # same tokens from the engine called directly (graph replay on: second call hits the captured graph)
    out2 = model.generate(**kw)
    assert out2[0, L:].tolist() == new
    model.use_graph = False
    out3 = model.generate(**kw)
    assert out3[0, L:].tolist() == new, "graph replay and eager launches must decode the same tokens"
    # EOS handling: make the first generated token an EOS -> generation stops right after it
    model.config._gen["eos_token_id"] = [new[0]]
    out4 = model.generate(**kw)
    assert out4.shape[1] == L + 1
    # errors the reference raises, kept: more <regionfeat> placeholders than boxes after the 100-box cap -> IndexError
    kw_bad = dict(kw)
    kw_bad["bbox_list"] = [kw["bbox_list"][0][:2]]
    with pytest.raises(IndexError):
        model.generate(**kw_bad)
    kw_oob = dict(kw)
    kw_oob["inputs"] = kw["inputs"].clone()
    kw_oob["inputs"][0, 0] = 151644            # a token id outside the 8192-row table: IndexError, not an out-of-bounds gather
    with pytest.raises(IndexError):
        model.generate(**kw_oob)


def test_unknown_checkpoint_key_and_unsupported_config_fail_loudly():
    from vlm_fo1.model import builder
    st = {"model.vision_tower.image_tower.x": torch.zeros(1), "model.something_else.weight": torch.zeros(1)}
    with pytest.raises(KeyError):
        builder.split_checkpoint(st)
    with pytest.raises(Exception):
        builder.split_checkpoint({"model.norm.weight": torch.zeros(1)})
    from vlm_fo1.model.fo1_model import FO1HFConfig
    bad = dict(CONFIG); bad["mm_region_feature_combination"] = "mean"
    with pytest.raises(NotImplementedError):
        FO1HFConfig(bad).engine_config()
    with pytest.raises(NotImplementedError):
        builder.load_pretrained_model("x/vlm-fo1_qwen2.5-vl", load_8bit=True)


def test_device_preprocessing_is_bit_identical_to_host_path():
    """rescale/normalise/patch layout on the GPU (fo1_patchify_u8_bf16, fo1_normalize_u8_bf16) from the resized
    uint8 image == the host processors' fp32 output cast to bf16, bit for bit, incl. the smart-resize and squash-resize cases."""
    import numpy as np
    from PIL import Image
    from vlm_fo1.model.image_processing import CLIPStyleAuxProcessor, Qwen2VLPatchProcessor
    rng = np.random.default_rng(7)
    for (w, h) in [(500, 399), (640, 480), (56, 56), (333, 711)]:
        img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB")
        host, dev = Qwen2VLPatchProcessor(), Qwen2VLPatchProcessor()
        dev.device = torch.device("cuda")
        a, b = host.preprocess(img, return_tensors="pt"), dev.preprocess(img, return_tensors="pt")
        assert torch.equal(a["image_grid_thw"], b["image_grid_thw"])
        assert b["pixel_values"].dtype == torch.bfloat16 and b["pixel_values"].is_cuda
        assert torch.equal(a["pixel_values"].to(torch.bfloat16), b["pixel_values"].cpu()), f"primary {w}x{h}"
        for mode in ("dynamic", "squash"):
            host, dev = CLIPStyleAuxProcessor(resize_mode=mode), CLIPStyleAuxProcessor(resize_mode=mode)
            dev.device = torch.device("cuda")
            a = host.preprocess(img, return_tensors="pt")["pixel_values"][0]
            b = dev.preprocess(img, return_tensors="pt")["pixel_values"][0]
            assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.to(torch.bfloat16), b.cpu()), f"aux {mode} {w}x{h}"


def test_two_requests_in_flight_through_the_dropin_model(tmp_path, monkeypatch):
    """FO1ForCausalLM.replica() + sharded_eval.request_workers: three worker threads, each with its own engine replica and HIP
    stream, generate for 6 requests; every answer equals the sequential one.  Both runs decode through the same route (the 128-slot
    pool, switched on before the sequential run): cross-route agreement is tests/test_decode_routes_gpu.py's, with an oracle and a
    margin."""
    from safetensors.torch import save_file
    from test_dropin_surface import ToyTokenizer
    from vlm_fo1 import mm_utils as MU
    from vlm_fo1.model import builder
    from vlm_fo1.task_templates import OD_template
    from vlm_fo1_amd import sharded_eval as SE
    model_dir = tmp_path / "VLM-FO1_Qwen2.5-VL-3B-v01"
    model_dir.mkdir()
    save_file({k: v.cpu().contiguous() for k, v in checkpoint_state().items()}, str(model_dir / "model.safetensors"))
    json.dump(CONFIG, open(model_dir / "config.json", "w"))

    class Tok(ToyTokenizer):
        def _enc(self, text):
            return [i % 8000 + 100 for i in super()._enc(text)]

    monkeypatch.setattr(builder, "_load_tokenizer", lambda p: Tok())
    monkeypatch.setattr(MU, "_IM_START_ID", 8190)
    monkeypatch.setattr(MU, "_IM_END_ID", 8191)
    monkeypatch.setattr(MU, "print", lambda *a, **k: None, raising=False)      # prepare_inputs prints every prompt (as the reference does)
    monkeypatch.setenv("FO1_DECODE_POOL", "128")
    monkeypatch.setenv("FO1_INFLIGHT", "3")
    tokenizer, model, procs = builder.load_pretrained_model(str(model_dir), device="cuda")
    paths = []
    for j, size in enumerate([(500, 399), (420, 280), (500, 399)]):
        p = str(tmp_path / f"img{j}.jpg")
        noise_image(size, 32 + 16 * j, seed=10 + j).convert("RGB").save(p)
        paths.append(p)
    boxes = [[161.0, 11.0, 292.0, 127.0], [268.0, 61.0, 428.0, 226.0], [12.0, 100.0, 140.0, 227.0], [30.0, 30.0, 90.0, 200.0]]
    reqs = [(paths[i % 3], boxes[: 2 + i % 3], ["orange", "apple", "cat"][i % 3]) for i in range(6)]

    def make_generate(m, stream):
        def generate(i):
            path, bl, word = reqs[i]
            messages = [{"role": "user", "content": [{"type": "image_url", "image_url": {"url": path}},
                                                     {"type": "text", "text": OD_template.format(word)}], "bbox_list": bl}]
            with torch.cuda.stream(stream):
                kw = MU.prepare_inputs(str(model_dir), m, procs, tokenizer, messages, max_tokens=6, top_p=0.05, temperature=0.0, do_sample=False)
                kw["streamer"] = None
                out = m.generate(**kw)
                return out[0, kw["inputs"].shape[1]:].tolist()
        return generate

    single = SE.request_workers(model, make_generate, n=1)      # switches the pool on: the sequential run decodes through it as well
    assert len(single) == 1 and model.engine._pool_svc is not None
    sequential = SE.run_sharded(len(reqs), [1.0] * len(reqs), single[0])
    workers = SE.request_workers(model, make_generate, n=3)
    assert len(workers) == 3
    overlapped = SE.run_sharded(len(reqs), [1.0] * len(reqs), workers)
    assert overlapped == sequential and all(t is not None and len(t) == 6 for _, t in sequential)
