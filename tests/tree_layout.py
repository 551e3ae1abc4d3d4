"""A tree buffer of include/qttt_tree.h, copied to the host and read as numpy arrays — by the layout written in that
header alone (game headers, node headers, 36 action slots, priors), not by the kernels' structs — and the comparison
of every byte of it that the header gives a meaning with the float64 model (tests/tree_model.py), before or after a
compaction.  Test infrastructure for tests/test_tree_whole_gpu.py, tests/test_tree_compact_gpu.py and
tests/test_selfplay_gpu.py; tests/test_tree_cpu.py checks the comparison itself.  A plain helper module."""
import numpy as np

GAME_BYTES, NODE_BYTES, PRIOR_BYTES = 128, 608, 144
CHILD_PAIR = 1 << 30
NODE_PRIORS, NODE_UNIFORM, NODE_TERMINAL, NODE_TURN = 1, 2, 4, 8
GAME_OVERFLOW, GAME_LEAF_TURN, GAME_LEAF_TERMINAL = 1, 2, 4

GAME_DTYPE = np.dtype({"names": ["used", "root", "depth", "leaf", "flags", "pad", "path_node", "path_action", "pad2"],
                       "formats": ["<i4", "<i4", "<i4", "<i4", "<u4", ("u1", (12,)), ("<i4", (10,)), ("u1", (10,)),
                                   ("u1", (46,))],
                       "offsets": [0, 4, 8, 12, 16, 20, 32, 72, 82], "itemsize": GAME_BYTES})
SLOT_DTYPE = np.dtype({"names": ["W", "N", "child"], "formats": ["<f8", "<u4", "<i4"], "offsets": [0, 8, 12],
                       "itemsize": 16})
NODE_DTYPE = np.dtype({"names": ["P", "Q", "legal", "Ntot", "flags", "slots"],
                       "formats": ["<u8", "<u8", "<u8", "<u4", "<u4", (SLOT_DTYPE, (36,))],
                       "offsets": [0, 8, 16, 24, 28, 32], "itemsize": NODE_BYTES})
assert GAME_DTYPE.itemsize == 128 and NODE_DTYPE.itemsize == 608


def tree_bytes(G, capacity):
    return G * (GAME_BYTES + capacity * (NODE_BYTES + PRIOR_BYTES))


def decode(buf, G, capacity):
    """buf: uint8 array of at least tree_bytes(G, capacity) bytes -> (games [G], nodes [G, capacity], priors f32
    [G, capacity, 36], tail = the bytes after the tree), all views of buf."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    o1 = G * GAME_BYTES
    o2 = o1 + G * capacity * NODE_BYTES
    o3 = o2 + G * capacity * PRIOR_BYTES
    assert buf.size >= o3
    games = buf[:o1].view(GAME_DTYPE)
    nodes = buf[o1:o2].view(NODE_DTYPE).reshape(G, capacity)
    priors = buf[o2:o3].view("<f4").reshape(G, capacity, 36)
    return games, nodes, priors, buf[o3:]


def pack_positions(recs, device="cuda:0", pack=None):
    """The packed planes (P, Q) u64[n] of positions given as oracle board records: one import_boards of all of them on
    `device`, or pack(the records as OracleBoards) where a test stands in for the device."""
    import oracle
    ob = oracle.OracleBoards.from_records(recs)
    if pack is not None:
        return pack(ob)
    import torch
    from qtttgym_amd import VecEnv
    env = VecEnv(ob.n, device=device)
    env.import_boards(ob.moves, ob.n_moves, ob.board, ob.qmask.astype(np.int16), ob.n_q)
    planes = env.state.view(torch.int64).view(2, -1)[:, :ob.n].cpu().numpy().view(np.uint64)
    return planes[0].copy(), planes[1].copy()


def _rows(mask):
    return np.argwhere(mask)[:8].tolist()


def assert_tree_equals_model(buf, G, capacity, model, sentinel, device="cuda:0", compacted=False, pack=None):
    """Every game header, every node < used and every network priors row of the tree buffer `buf` (host bytes) against
    the model; what the header leaves unwritten must still hold the byte `sentinel` that the test filled the buffer
    with before qttt_tree_reset: the headers' padding, whatever follows the tree in buf and, unless `compacted`, the
    node records and priors rows at or beyond `used` and the priors rows of nodes without network priors (a compaction
    leaves those unspecified).  Returns the number of network priors rows compared."""
    games, nodes, priors, tail = decode(buf, G, capacity)
    dump = model.dump()
    assert len(dump) == G
    used = np.array([d["used"] for d in dump], dtype=np.int32)
    assert (used <= capacity).all()
    live = np.arange(capacity)[None, :] < used[:, None]
    dev, pri = nodes[live], priors[live]                  # nodes < used, flattened over the games in (game, node) order
    flat = [n for d in dump for n in d["nodes"]]
    assert len(flat) == len(dev)
    assert all(len(c) < 2 or c[1] == c[0] + 1 for n in flat for c in n["children"])
    leaves = [d["nodes"][d["leaf"]] for d in dump]
    P, Q = pack_positions([n["rec"] for n in flat], device, pack)
    network = np.array([isinstance(n["P"], np.ndarray) for n in flat], dtype=bool)
    expected = (
        ("used", games["used"], used),
        ("root", games["root"], np.array([d["root"] for d in dump], dtype=np.int32)),
        ("depth", games["depth"], np.array([len(d["path"]) for d in dump], dtype=np.int32)),
        ("leaf", games["leaf"], np.array([d["leaf"] for d in dump], dtype=np.int32)),
        ("game flags", games["flags"],
         np.array([(GAME_OVERFLOW if d["overflow"] else 0) | (GAME_LEAF_TURN if n["turn"] else 0)
                   | (GAME_LEAF_TERMINAL if n["terminal"] else 0) for d, n in zip(dump, leaves)], dtype=np.uint32)),
        ("P", dev["P"], P),
        ("Q", dev["Q"], Q),
        ("legal", dev["legal"], np.array([n["legal"] for n in flat], dtype=np.uint64)),
        ("Ntot", dev["Ntot"], np.array([n["Ntot"] for n in flat], dtype=np.uint32)),
        ("flags", dev["flags"],
         np.array([(0 if n["P"] is None else NODE_PRIORS) | (NODE_UNIFORM if isinstance(n["P"], str) else 0)
                   | (NODE_TERMINAL if n["terminal"] else 0) | (NODE_TURN if n["turn"] else 0)
                   | ((n["winner"] + 1) << 8) for n in flat], dtype=np.uint32)),
        ("N", dev["slots"]["N"], np.array([n["N"] for n in flat], dtype=np.uint32).reshape(-1, 36)),
        ("W", dev["slots"]["W"].view(np.int64),                                                     # bit for bit
         np.array([n["W"] for n in flat], dtype=np.float64).reshape(-1, 36).view(np.int64)),
        ("child", dev["slots"]["child"],
         np.array([[-1 if not c else (c[0] | (CHILD_PAIR if len(c) == 2 else 0)) for c in n["children"]] for n in flat],
                  dtype=np.int32).reshape(-1, 36)),
        ("network priors", pri[network].view(np.uint32),                                            # bit for bit
         np.array([n["P"] for n in flat if isinstance(n["P"], np.ndarray)], dtype=np.float32).reshape(-1, 36)
         .view(np.uint32)))
    for name, got, ref in expected:
        assert np.array_equal(got, ref), (name, _rows(got != ref))
    for g, d in enumerate(dump):
        for k, (i, a) in enumerate(d["path"]):
            assert games["path_node"][g, k] == i and games["path_action"][g, k] == a, ("path", g, k)
    unwritten = [("the game headers' padding", games["pad"]), ("the game headers' padding", games["pad2"]),
                 ("bytes after the tree", tail)]
    if not compacted:
        unwritten += [("a priors row of a node without network priors", pri[~network]),
                      ("a priors row at or beyond `used`", priors[~live]),
                      ("a node record at or beyond `used`", nodes[~live])]
    for name, region in unwritten:
        assert (region.view(np.uint8) == sentinel).all(), name + ": written"
    return int(network.sum())
