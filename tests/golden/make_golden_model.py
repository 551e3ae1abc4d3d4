#!/usr/bin/env python3
"""Generates tests/golden/model_eval.npz from the UNMODIFIED reference's network (`nn.py`: Model, get_mask, forward)
and its trained weights (`model.pt`), loaded through ref_shim.py.  Build container only; the .npz is data.

Positions: the 260 parents of expand_traces.npz, then distinct children of their expansions (first come, by the
reference's hash) up to N_POSITIONS in all.  For each: the Board attributes (import_boards form), the reference
AlphaZero.GameState.to_vector() fed to Model.forward (alphazero.py:294-300) -> value, logits (with the −inf mask),
and torch.softmax(logits) = Categorical(logits).probs.  Also model.pt's ten tensors as f32 arrays.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shim import load_reference, REFERENCE_ROOT  # noqa: E402

N_POSITIONS = 800                    # the weights are ~0.7 MB compressed: the file stays well under 1 MB
KEYS = ("fc.0.weight", "fc.0.bias", "fc.2.weight", "fc.2.bias", "fc.4.weight", "fc.4.bias",
        "V_head.1.weight", "V_head.1.bias", "pi_head.1.weight", "pi_head.1.bias")


def main():
    load_reference()
    sys.path.insert(0, REFERENCE_ROOT)
    import torch
    import alphazero as ref_az                   # the reference's alphazero.py / nn.py, unmodified
    import nn as ref_nn
    sd = torch.load(os.path.join(REFERENCE_ROOT, "model.pt"), map_location="cpu")
    model = ref_nn.Model()
    model.load_state_dict(sd)
    model.eval()

    ex = np.load(os.path.join(HERE, "expand_traces.npz"))
    rows = [(ex["p_board"][i], ex["p_moves"][i], ex["p_n_moves"][i], ex["p_qmask"][i], ex["p_n_q"][i])
            for i in range(len(ex["p_board"]))]
    seen = {(tuple(r[0]), tuple(map(tuple, r[1][:r[2]]))) for r in rows}
    nc = ex["n_children"]
    for e in range(len(nc)):
        for c in range(int(nc[e])):
            r = (ex["c_board"][e, c], ex["c_moves"][e, c], ex["c_n_moves"][e, c], ex["c_qmask"][e, c],
                 ex["c_n_q"][e, c])
            key = (tuple(r[0]), tuple(map(tuple, r[1][:r[2]])))
            if key in seen or len(rows) >= N_POSITIONS:
                continue
            seen.add(key)
            rows.append(r)

    GS = ref_az.AlphaZero.GameState
    values, logits, vectors = [], [], []
    for board, moves, n_moves, qmask, n_q in rows:
        gs = GS([int(x) for x in board], [(int(m[0]), int(m[1]), t) for t, m in enumerate(moves[:n_moves])],
                int(n_moves) % 2 == 0, None, False)
        gs.qstructs = [{v for v in range(9) if int(qmask[k]) >> v & 1} for k in range(int(n_q))]
        vec = gs.to_vector()
        with torch.no_grad():
            v, lg = model.forward(vec)
        vectors.append(vec)
        values.append(float(v))
        logits.append(lg.numpy())
    logits = np.array(logits, dtype=np.float32)
    probs = torch.softmax(torch.from_numpy(logits), -1).numpy()

    out = {k.replace(".", "_"): sd[k].numpy().astype(np.float32) for k in KEYS}
    out.update({
        "board": np.array([r[0] for r in rows], dtype=np.int8), "moves": np.array([r[1] for r in rows], dtype=np.uint8),
        "n_moves": np.array([r[2] for r in rows], dtype=np.uint8), "qmask": np.array([r[3] for r in rows], dtype=np.uint16),
        "n_q": np.array([r[4] for r in rows], dtype=np.uint8),
        "value": np.array(values, dtype=np.float32), "logits": logits, "probs": probs.astype(np.float32),
        "vector": np.array(vectors, dtype=np.float32),
    })
    path = os.path.join(HERE, "model_eval.npz")
    np.savez_compressed(path, **out)
    allm = int(np.isneginf(logits).all(1).sum())
    print("wrote %s: %d positions (%d parents, %d all-masked rows, %d of them parents), %d B"
          % (path, len(rows), len(ex["p_board"]), allm, int(np.isneginf(logits[:len(ex["p_board"])]).all(1).sum()),
             os.path.getsize(path)))


if __name__ == "__main__":
    main()
