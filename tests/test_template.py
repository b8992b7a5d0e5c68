"""Family scaffolding generator test (mirror reference template codegen)."""
import importlib
import sys

import torch


def test_generated_family_decodes(tmp_path):
    from bloombee_amd.models.template import generate_family

    d = generate_family(
        "bloombee_amd/models/template/spec_llama.yaml", str(tmp_path))
    sys.path.insert(0, str(tmp_path))
    try:
        importlib.import_module("myllama")
        from bloombee_amd.engine import LocalEngine

        eng = LocalEngine("myllama-tiny", device="cpu", seed=0,
                          kv_max_tokens=4096)
        ids = torch.randint(0, 900, (1, 6),
                            generator=torch.Generator().manual_seed(2))
        out = eng.generate_greedy(ids, 4)
        assert out.shape == (1, 4)
        # decode == prefill consistency on the generated block
        kv1 = eng.kv_pool.allocate(1, 64)
        full = eng.prefill(ids, kv1)
        kv1.close()
        kv2 = eng.kv_pool.allocate(1, 64)
        tok = eng.prefill(ids[:, :1], kv2)
        for t in range(1, 6):
            tok = eng.decode_step(ids[0, t].view(1), kv2)
        kv2.close()
        assert torch.equal(full, tok)
    finally:
        sys.path.remove(str(tmp_path))


def test_generated_family_mixed_device(tmp_path):
    """A generated family handles mixed-device sessions: decode hidden states
    with the committed KV moved to a host prefix match the never-swapped
    run's. Before the generated block went through block_common's
    rotary_positions / paged_attention_qkv it ignored the host prefix and
    this comparison failed (max|diff| 0.0725 at max|dense| 0.0771)."""
    from bloombee_amd.models.template import generate_family
    from mixed_device_scenario import decode_hidden, make_engine
    from test_mixed_device_families import assert_hidden_match

    generate_family(
        "bloombee_amd/models/template/spec_llama.yaml", str(tmp_path))
    sys.path.insert(0, str(tmp_path))
    try:
        importlib.import_module("myllama")
        eng = make_engine("myllama-tiny")
        dense = decode_hidden(eng, swapped=False)
        mixed = decode_hidden(eng, swapped=True)
        assert_hidden_match(dense, mixed)
    finally:
        sys.path.remove(str(tmp_path))
