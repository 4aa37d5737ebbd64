"""M8's 256 x 256 kernel (csrc/gemm_split_big.hip) on grids of more than one round of blocks (one block per CU, 256 CUs): the
existing bit test of the one-block-per-CU kernels never exceeds 24 tiles.

Shapes (G, M, K, N), tiles of 256 x 256:
  (36, 2060, 64, 512)   648 tiles = three rounds, ragged last row block, two K steps
  (5, 4100, 96, 1024)   340 tiles = two rounds, odd K-step count (the lateral products' K)
  (1, 256, 512, 256)    one tile
  (5, 4100, 512, 1024)  340 tiles and 16 K steps: a K loop as long as the Winograd-domain products'
For each: pipe=3 (the big kernel, forced) against pipe=0 (the 128 x 128 single-stage kernel) with torch.equal, fp16 x 2 and
bf16 x 2, plain / bias + ReLU / out_amax (tensor and word); a second call and a captured-graph replay give the first call's bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(36, 2060, 64, 512), (5, 4100, 96, 1024), (1, 256, 512, 256), (5, 4100, 512, 1024)]


@pytest.fixture(scope="module")
def N():
    from semseg import _native
    _native.lib()
    return _native


@pytest.mark.parametrize("G,M,K,Nn", SHAPES)
def test_rounds_of_256x256_tiles_give_the_bits_of_the_128x128_kernel(N, G, M, K, Nn):
    g = torch.Generator(device="cuda").manual_seed(G + M + K + Nn)
    A = torch.randn(G, M, K, generator=g, device="cuda") * torch.exp2(torch.randint(-6, 3, (G, M, 1), generator=g, device="cuda").float())
    W = torch.randn(G, Nn, K, generator=g, device="cuda") / K ** 0.5
    bias = torch.randn(Nn, generator=g, device="cuda")
    packed = {terms: N.gemm_split_pack(W, terms=terms) for terms in (22, 2)}

    def variants(pipe):
        outs = {}
        for terms, Wp in packed.items():
            outs[terms, "plain"] = N.gemm_split(A, Wp, groups=1, pipe=pipe)
            outs[terms, "bias_relu"] = N.gemm_split(A, Wp, bias=bias, relu=True, groups=1, pipe=pipe)
        word = N.amax_word(A.device)
        outs[22, "out_amax"] = N.gemm_split(A, packed[22], out_amax=word, groups=1, pipe=pipe).clone()
        outs[22, "out_amax_word"] = word.clone()
        return outs

    o0 = variants(0)
    o3 = variants(3)
    again = variants(3)
    for key, a in o0.items():
        assert torch.equal(a, o3[key]), (key, (a.float() - o3[key].float()).abs().max().item())
        assert torch.equal(o3[key], again[key]), ("second call", key)
    assert o3[22, "out_amax_word"].item() == o3[22, "out_amax"].abs().max().view(torch.int32).item()

    # a captured launch replays to the same bits (out and the scale words are the graph's own buffers)
    out = torch.empty(G, M, Nn, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        N.gemm_split(A, packed[22], bias=bias, relu=True, groups=1, pipe=3, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        N.gemm_split(A, packed[22], bias=bias, relu=True, groups=1, pipe=3, out=out)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, o3[22, "bias_relu"])
