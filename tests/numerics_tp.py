"""Helpers of the tensor-parallel serving tests (tests/test_serving_tp.py, tests/test_serving_tp_gpu.py):
the tiny model whose local shapes land on and off the K multiples of the quantised-weight kernels, which
of its projections get codes on a rank, the prompt and the feature matrix of ``generate``.

The model: 2 layers, head_dim 64, d = 64 heads, ffn 512, vocab 97, at heads 2 and 3 over two ranks and
heads 6 over four.  What a rank then holds (K is the last dimension):

    heads  TP  local heads  QKV [192 h, d]  Wo [d, 64 h]  gate|up [1024 / TP, d]  down [d, 512 / TP]  lm_head
      2    2     1, 1       K 128           K 64          K 128                   K 256               [48 | 49, 128]
      3    2     2, 1       K 192           K 128 | 64    K 192                   K 256               [48 | 49, 192]
      6    4   2, 2, 1, 1   K 384           K 128 | 64    K 384                   K 128               [24 x 3 | 25, 384]

fp8 codes need K % 64 == 0: all 9 projections on every rank.  MXFP4 codes need K % 128 == 0: heads 2, TP 2:
all but Wo, 7 and 7; heads 3, TP 2: Wo and down on rank 0, down alone on rank 1, 4 and 2; heads 6, TP 4:
all 9 on ranks 0 and 1, all but Wo on ranks 2 and 3, 9, 9, 7, 7.  At TP 1 (d = 128, 192, 384; down K 512):
9, 2 (the down projections) and 9."""
import torch

LAYERS, HEAD_DIM, FFN, VOCAB, MAXLEN = 2, 64, 512, 97, 64
B, T, NEW = 3, 12, 8
WORLD_HEADS = ((2, 2), (2, 3), (4, 6))            # (TP world, heads) of the multi-rank runs
K_MULTIPLE = {"fp8": 64, "mxfp4": 128}            # weight_dtype -> the K multiple its kernel takes
# codes per rank: {weight_dtype: {(world, heads): [count on rank 0, ...]}} (the table above)
CODED_COUNTS = {
    "fp8": {(1, 2): [9], (1, 3): [9], (1, 6): [9], (2, 2): [9, 9], (2, 3): [9, 9], (4, 6): [9, 9, 9, 9]},
    "mxfp4": {(1, 2): [9], (1, 3): [2], (1, 6): [9], (2, 2): [7, 7], (2, 3): [4, 2], (4, 6): [9, 9, 7, 7]},
}


def tp_model(heads, vocab=VOCAB):
    """This rank's shard of the RMSNorm model above (fp32 parameters on the CPU), seed 0."""
    from distributed_pytorch_from_scratch_amd.models import ModelArgs, Transformer
    from distributed_pytorch_from_scratch_amd.utils.dist import set_seed
    m = Transformer.from_args(ModelArgs(attn_dim=HEAD_DIM * heads, ffn_dim=FFN, num_heads=heads, num_layers=LAYERS,
                                        vocab_size=vocab, maxlen=MAXLEN, vocab_pad_to=1))
    set_seed(0)
    m.reset_parameters()
    return m.eval()


def prompt(b=B, t=T, seed=5, vocab=VOCAB):
    return torch.randint(3, vocab, (b, t), generator=torch.Generator().manual_seed(seed))


def projections(model):
    """The ``4 * layers + 1`` projection weights of the decode step, named, in the order of the step's
    session: the lm_head, then QKV, Wo, gate|up and down of every layer."""
    out = [("lm_head", model.lm_head.weight)]
    for li, layer in enumerate(model.layers):
        out += [(f"{li}.wqkv", layer.attn.wqkv.weight), (f"{li}.wo", layer.attn.wo.weight),
                (f"{li}.wgu", layer.ffn.gate_up.weight), (f"{li}.wd", layer.ffn.down_proj.weight)]
    return out


def coded(model, weight_dtype):
    """The names of the projections of this rank that get codes under ``weight_dtype``: those whose local
    K is a multiple of what the format's kernel takes.  From the parameter shapes alone."""
    return [name for name, w in projections(model) if w.size(1) % K_MULTIPLE[weight_dtype] == 0]


def coded_names(model, codes):
    """The names of the projections that ``codes`` (a ``quantise_weights`` result) holds, and nothing else."""
    names = {id(w): name for name, w in projections(model)}
    assert set(codes) <= set(names), "quantise_weights holds a tensor that is no projection weight"
    return [name for name, w in projections(model) if id(w) in codes]


ROWS = dict(prompt_lens=[12, 7, 9], temperature=[0.0, 0.8, 1.0], top_k=20, seed=3)
# (name, generate kwargs); CODED names the entries whose decode steps read weight codes
MATRIX = [
    ("plain", {}),
    ("kv8", dict(kv_dtype="fp8")),
    ("paged", dict(kv_page=16)),
    ("kv8_paged", dict(kv_dtype="fp8", kv_page=16)),
    ("w8", dict(weight_dtype="fp8")),
    ("w4", dict(weight_dtype="mxfp4")),
    ("all", dict(weight_dtype="mxfp4", kv_dtype="fp8", kv_page=16, **ROWS)),
    ("pen", dict(temperature=[0.0, 0.8, 1.0], seed=3, repetition_penalty=1.3, presence_penalty=0.2,
                 frequency_penalty=0.1, return_logprobs=True)),
]
CODED = ("w8", "w4", "all")
