"""Writes attention_long.npz / attention_long.json: the reference's AudioEncoder (small channel counts) + AttentionModel at
visible_steps = 100 (sequence_length 128, head size 64: one head of 64 channels), one training step per score function and branch.

Run from the repository root with the reference checkout importable (see generate_golden.py, whose stubs and helpers this reuses):
    python tests/golden/generate_attention_long.py
Only inputs and outputs are stored: parameters, the batch, the forward outputs, the losses of four runs (softplus / linear scores, the
default branch and all timesteps) and the parameter gradients of two of them (softplus default branch, linear all timesteps).
"""
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)


def gen_attention_long():
    from attention_model import AttentionModel
    C, H, K, V, B, layers, heads, ff = 64, 16, 12, 100, 2, 2, 1, 32
    L = 465 + (V + K) * 160 + 11
    enc_channels = [8, 8, 8, 8, C]
    ar_dict = {'channels': C, 'num_layers': layers, 'num_heads': heads, 'feedforward_size': ff, 'dropout': 0.0,
               'sequence_length': 128, 'output_size': H}
    scale = {f"encoder.layers.{l}.weight": s for l, s in enumerate([4.0, 3.0, 3.0, 3.0, 2.0])}
    scale["autoregressive_model.end_layer.weight"] = 1.5

    def build():
        torch.manual_seed(31)
        enc = G.ref_model.AudioEncoder({'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': enc_channels,
                                        'bias': True})
        ar = AttentionModel(ar_dict)
        model = G.ref_model.AudioPredictiveCodingModel(enc, ar, enc_size=C, ar_size=H, visible_steps=V, prediction_steps=K)
        g = torch.Generator().manual_seed(37)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n in scale:
                    p.mul_(scale[n])
                if n.startswith("autoregressive_model."):      # as in generate_golden.gen_attention: the default init would hide mix-ups
                    if ".norm" in n and n.endswith("weight"):
                        p.add_(0.3 * torch.randn(p.shape, generator=g))
                    elif n.endswith("bias"):
                        p.add_(0.2 * torch.randn(p.shape, generator=g))
                    elif "encoder.layers" in n:
                        p.mul_(1.0 + 0.5 * torch.rand(p.shape, generator=g))
        return model

    out = {}
    model = build()
    for k, v in G.np_state(model).items():
        if not k.endswith("positional_encoder.pe"):        # a fixed table, rebuilt by the module
            out["param/" + k] = v
    g = torch.Generator().manual_seed(41)
    data = torch.randn(B, L, generator=g) * 0.5
    out["data"] = data.numpy()
    with torch.no_grad():
        pz, tg, z, c = model(data.unsqueeze(1))
        out["fwd/predicted_z"], out["fwd/c"] = pz.numpy(), c.numpy()
    meta = {"C": C, "H": H, "K": K, "V": V, "B": B, "L": L, "enc_channels": enc_channels, "ar": ar_dict, "runs": []}
    runs = (("softplus", G.ref_train.softplus_score_function, False, 1.0, True),
            ("linear", G.ref_train.linear_score_function, True, 0.01, True),
            ("softplus", G.ref_train.softplus_score_function, True, 0.5, False),
            ("linear", G.ref_train.linear_score_function, False, 0.1, False))
    for rid, (fn_name, fn, all_t, reg, keep_grads) in enumerate(runs):
        model = build()
        ds = G.TensorDataset(data)
        logger = G.Logger()
        with G.quiet():
            tr = G.ref_train.ContrastiveEstimationTrainer(model=model, dataset=ds, logger=logger, device=None, regularization=reg,
                                                          score_over_all_timesteps=all_t, score_function=fn, prediction_steps=K,
                                                          ar_size=H)
            random.seed(77)
            tr.train(batch_size=B, epochs=1, lr=1e-4, num_workers=0, max_steps=1)
        tag = f"run{rid}"
        meta["runs"].append({"tag": tag, "score": fn_name, "all_timesteps": all_t, "reg": reg, "batch": ds.accessed[:B],
                             "loss": logger.loss_meter.values[0], "grads": keep_grads})
        if keep_grads:
            for n, p in model.named_parameters():
                out[f"{tag}/grad/{n}"] = p.grad.numpy().copy()
    np.savez_compressed(os.path.join(G.OUT, "attention_long.npz"), **out)
    with open(os.path.join(G.OUT, "attention_long.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("attention_long:", [(r["score"], r["all_timesteps"], r["loss"]) for r in meta["runs"]])


if __name__ == "__main__":
    gen_attention_long()
