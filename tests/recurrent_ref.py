"""The numpy float64 statement of the recurrent head (include/dynenv.h, dynenv_recurrent_head; the tail of the reference's
DynEnvFeatureExtractor.forward, DynEnv/models/models.py:584-594, 610-616, and its LSTMLayer, models.py:16-95) that the tests compare
against, and the parameters they share.  A helper module: no tests.

For row p of environment p // A:
  x = feat when ext is None, else LayerNorm(leaky(cat(feat, ext) W_tr^T + b_tr; 0.1); TransformNet.2)
  h, c = 0 where reset_env[p // A], without being looked at
  g = x W_ih^T + b_ih + h W_hh^T + b_hh, torch's gate order i, f, g, o
  c' = sigmoid(g_f) c + sigmoid(g_i) tanh(g_g);  h' = sigmoid(g_o) tanh(c');  out = LayerNorm(h'; bn)"""
import numpy as np

NAMES = ("TransformNet.0.weight", "TransformNet.0.bias", "TransformNet.2.weight", "TransformNet.2.bias", "LSTM.cell.weight_ih",
         "LSTM.cell.weight_hh", "LSTM.cell.bias_ih", "LSTM.cell.bias_hh", "LSTM.transformer.0.weight", "LSTM.transformer.0.bias", "bn.weight",
         "bn.bias")
EPS = 1e-5
SLOPE = 0.1


def make_params(F, X, seed=0):
    """{name: float32 array} of a GpuRecurrentHead(F, ., ., X): torch's default initialisation, then EVERY bias and LayerNorm bias
    uniform in +-0.5 and the LayerNorm weights in [0.5, 1.5] (a LayerNorm starts at weight 1, bias 0: a forgotten one would be invisible)"""
    import torch
    from dynenv_amd import GpuRecurrentHead
    gen = torch.Generator().manual_seed(2000 + seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    layer = GpuRecurrentHead(F, 1, 1, X)
    torch.random.set_rng_state(state)
    with torch.no_grad():
        for k, p in layer.named_parameters():
            if k in ("bn.weight", "TransformNet.2.weight"):
                p.copy_(torch.rand(p.shape, generator=gen) + 0.5)
            elif "bias" in k:
                p.copy_(torch.rand(p.shape, generator=gen) - 0.5)
    return {k: v.detach().numpy().copy() for k, v in layer.state_dict().items()}


def load(module, params, dtype=None):
    """the parameters into a GpuRecurrentHead (or anything with the reference's names), strict"""
    import torch
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    return module if dtype is None else module.to(dtype)


def layer_norm(x, w, b):
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + EPS) * w + b


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def head_step(feat, ext, h, c, reset_env, A, params):
    """feat [P, F], ext [P, X] or None, h and c [P, F] (rows of a reset environment are not looked at), reset_env [E] or None ->
    float64 (h', c', out)"""
    g = lambda name: np.asarray(params[name], np.float64)  # noqa: E731
    x = np.asarray(feat, np.float64)
    P, F = x.shape
    if ext is not None:
        x = np.concatenate([x, np.asarray(ext, np.float64)], 1) @ g("TransformNet.0.weight").T + g("TransformNet.0.bias")
        x = layer_norm(np.where(x > 0, x, SLOPE * x), g("TransformNet.2.weight"), g("TransformNet.2.bias"))
    h, c = np.array(h, np.float64), np.array(c, np.float64)
    if reset_env is not None:
        rows = np.repeat(np.asarray(reset_env).astype(bool), A)
        h[rows] = 0.0
        c[rows] = 0.0
    gates = x @ g("LSTM.cell.weight_ih").T + g("LSTM.cell.bias_ih") + h @ g("LSTM.cell.weight_hh").T + g("LSTM.cell.bias_hh")
    i, f, gg, o = (gates[:, k * F:(k + 1) * F] for k in range(4))
    c2 = sigmoid(f) * c + sigmoid(i) * np.tanh(gg)
    h2 = sigmoid(o) * np.tanh(c2)
    return h2, c2, layer_norm(h2, g("bn.weight"), g("bn.bias"))
