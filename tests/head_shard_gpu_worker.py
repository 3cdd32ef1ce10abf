"""Worker of tests/test_gpu_head_shard.py: one of G ranks that all sit on cuda:0 (a 1-GPU box) and talk over gloo.
Drives two stacked Llama attention layers through slime_amd.dist.head_sharded_attention with ops.llama_attention_forward_resid (rank 0,
which carries the residual) / ops.llama_attention_forward (the other ranks) as the local call, in the shape of bench.py's ``run()``:
rank 0 writes into ping-pong buffers, the other ranks get fresh tensors, hidden is resid.  World 2 runs (1024, 8, 2), world 4
(512, 4, 4); both dtypes in one run.  Asserts
 (a) after each layer every rank holds the same bits (all-gather and compare);
 (b) layer 1's result is inside head_shard_conformance's bound (2) of the float64 sum of the ranks' terms, which every rank computes
     itself, in process, from the full layer's weights;
 (c) after two layers the result is within the per-stage tolerance, applied per layer and hence doubled, of the oracle's two layers."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

GEOM = {2: (1024, 8, 2, 2), 4: (512, 4, 4, 4)}
BATCH, S = 2, 65


def main():
    import head_shard_conformance as HS
    from slime_amd import dist as D, ops
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    hidden, hq, hkv, _ = geom = GEOM[world]
    assert geom[3] == world
    fails = []
    for dtype in HS.DTYPES:
        tag = f"world {world} {HS.DT_ID[dtype]} rank {rank}"
        layers = [HS.layer_weights(hidden, hq, hkv, seed) for seed in (7, 8)]
        pack = lambda sl: ops.pack_llama_attention(sl[0], sl[1], sl[2], sl[3], sl[4], sl[5], dtype, dev)
        first = [pack(sl) for sl in HS.rank_slices(layers[0], hq, hkv, world)]          # every rank's slice of layer 1, for (b)
        mine = [first[rank], pack(HS.rank_slices(layers[1], hq, hkv, world)[rank])]
        x0, _, pos = HS.layer_inputs(hidden, BATCH, S, dtype)
        start, length = HS.kv_ranges("right", BATCH, S)
        mask = HS.range_mask(start, length, BATCH, S).to(dev)
        x0, pos_d = x0.to(dev).view(BATCH, S, hidden), pos.to(dev).view(BATCH, S)
        bufs = [torch.empty((BATCH, S, hidden), dtype=dtype, device=dev) for _ in range(2)]

        def local(h, r, p, i):
            if r is not None:
                return ops.llama_attention_forward_resid(p, h, r, pos_d, mask, out=bufs[i & 1])
            return ops.llama_attention_forward(p, h, pos_d, mask, dtype)

        x, results = x0, []
        for i, p in enumerate(mine):
            x = D.head_sharded_attention(lambda h, r, p=p, i=i: local(h, r, p, i), x, x)
            assert x.dtype == dtype and tuple(x.shape) == (BATCH, S, hidden)
            results.append(x.clone())
            everyone = [torch.empty_like(x) for _ in range(world)]
            dist.all_gather(everyone, x.contiguous())
            for r, other in enumerate(everyone):                                           # (a)
                if not torch.equal(other.view(torch.int16), x.view(torch.int16)):
                    fails.append(f"{tag}: after layer {i + 1} rank {r} holds other bits")
        # (b) the terms of layer 1, in process
        terms = [ops.llama_attention_forward_resid(first[0], x0, x0, pos_d, mask)]
        terms += [ops.llama_attention_forward(first[r], x0, pos_d, mask, dtype) for r in range(1, world)]
        torch.cuda.synchronize()
        ratio = HS.worst_ratio(results[0].double() - HS.float64_sum(terms), HS.reduce_bound(terms, dtype))
        if not ratio <= 1.0:
            fails.append(f"{tag}: layer 1 leaves the reduce bound, worst |err| / bound {ratio:.3f}")
        # (c) two layers against the oracle
        flat = lambda t: t.reshape(BATCH * S, hidden)
        y = flat(x0)
        for w in layers:
            y = HS.oracle_layer(w, hq, hkv, y, y, pos, start, length, BATCH, S)
        rel = float((flat(results[1]).double().cpu() - y).norm() / y.norm())
        if not rel < 2 * HS.TOL[dtype]:
            fails.append(f"{tag}: two layers rel-L2 {rel:.3e} against the oracle, tolerance {2 * HS.TOL[dtype]:.1e}")
        if rank == 0:
            print(f"world {world} {HS.DT_ID[dtype]}: reduce worst |err| / bound {ratio:.3f}; two layers rel-L2 vs oracle {rel:.3e} "
                  f"(tolerance {2 * HS.TOL[dtype]:.1e})", flush=True)
    for f in fails:
        print(f, flush=True)
    flag = torch.tensor([0 if fails else 1])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) == 1 else 3)


if __name__ == "__main__":
    main()
