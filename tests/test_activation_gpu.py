"""GPU: the encoder with activation='relu' and 'tanh' (ReLU = activation code 1 with slope 0, tanh = code 2; include/voxactb_hip.h).

Against reference fixtures (tests/golden/make_golden_activation.py, F17a / F17c): Q-values within 1e-4, the loss within 1e-4, every
parameter-gradient norm and the small gradients element-wise within 3e-3 -- in exact 'fp32' and in the default precision.  Then every new
kernel mode against float64 PyTorch, and two agents of different activations interleaved in one process."""
import numpy as np
import pytest
import torch

from oracle import weights as ow
from voxactb_amd import ops, synthetic
from voxactb_amd.agents.peract_bc import launch_utils as lu
from voxactb_amd.agents.peract_bc.perceiver_lang_io import PerceiverVoxelLangEncoder, PerceiverVoxelLang2RobotsEncoder

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_Q = 1e-4
GRAD_TOL = 3e-3
# cache key of the saved activation output per kink site (make_golden.py: KINK_SITES)
KINK_KEYS = {'input_preprocess': 'd0', 'patchify': 'patch', 'up0.conv_up.0': 'z1', 'up0.conv_up.2': 'u0', 'final': 'u'}
KINK_FLIP_FRACTION = 5e-5       # as tests/test_c2_reference_gpu.py
KINK_FLIP_MARGIN = 3e-5


def T(a):
    return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).abs().max())


def force_relu_kinks(cache, g):
    """ReLU twin of test_c2_reference_gpu.force_kinks: the backward at the reference run's subgradient choices.  A saved ReLU output
    carries no magnitude below zero (it is 0), so the forced value is 1e-30 where the reference's pre-activation was positive and 0
    where it was not -- ReLU' gates on the output being > 0, here and in PyTorch.  Guards: the listed elements are near zero in the
    product too, the flipped ones are a vanishing fraction, and a product value > 0 the reference calls negative is within
    tau + KINK_FLIP_MARGIN of zero.  Returns the number of flipped choices."""
    flips = 0
    tau = float(g['kink_tau'])
    for site, key in KINK_KEYS.items():
        k = 'kink__%s__idx' % site
        if k not in g.files or key not in cache:
            continue
        idx = T(g[k]).long().to(DEV)
        if idx.numel() == 0:
            continue
        pos = T(g['kink__%s__pos' % site]).to(DEV) > 0
        flat = cache[key].view(-1)
        cur = flat[idx]
        assert float(cur.abs().max()) < 1e-3, (site, float(cur.abs().max()))
        assert float(cur.min()) >= 0.0, site                      # a ReLU output
        diff = (cur > 0) != pos
        n = int(diff.sum())
        if n:
            assert n <= max(4, KINK_FLIP_FRACTION * flat.numel()), (site, n, flat.numel())
            assert float(cur[diff].max()) <= tau + KINK_FLIP_MARGIN, (site, n)
        flips += n
        flat[idx] = torch.where(pos, torch.full_like(cur, 1e-30), torch.zeros_like(cur))
    return flips


def replay(g, arm):
    B, H, W, V = int(g['cfg_B']), int(g['cfg_H']), int(g['cfg_W']), int(g['cfg_V'])
    cams = [str(c) for c in g['cfg_cams']]
    rs = synthetic.make_replay_sample(B, cams, (H, W), V, int(g['cfg_low_dim']), seed=1, arm_pred_loss=arm)
    rs = {k: (v[:, 0] if v.dim() > 2 else v) for k, v in rs.items()}
    return {k: ((v.float() / 255.0) * 2.0 - 1.0 if 'rgb' in k else v.float()) for k, v in rs.items()}


def check_grads(enc, g):
    P = dict(enc.named_parameters())
    bad = []
    for n, rn in zip([str(n) for n in g['grad_names']], T(g['grad_norms'])):
        gn = float(P[n].grad.norm())
        if abs(gn - float(rn)) > GRAD_TOL * float(rn) + 1e-5:
            bad.append((n, gn, float(rn)))
        key = 'grad__' + n
        if key in g.files:
            ref = T(g[key])
            e = maxerr(P[n].grad, ref)
            if e > GRAD_TOL * float(ref.abs().max()) + 1e-5:
                bad.append((n, 'full', e, float(ref.abs().max())))
    assert not bad, bad


def heads_loss(q, o, trans, rot_grip, coll, B, V):
    at = trans.long()
    lab = ((at[:, 0] * V + at[:, 1]) * V + at[:, 2]).int().to(DEV)
    dq = torch.empty((B, V ** 3), device=DEV)
    l_t, _, _ = ops.ce_big(q.reshape(B, -1), lab, dq, 1.0 / B)
    labs = torch.cat([rot_grip.int(), coll.int()[:, :1]], 1).to(DEV).contiguous()
    d_o = torch.empty_like(o)
    l_h, _ = ops.ce_rows(o, [(0, 72), (72, 72), (144, 72), (216, 2), (218, 2)], labs, d_o, 1.0 / B)
    return l_t + l_h.sum(1), dq, d_o


def run_fixture(g, precision):
    activation = str(g['cfg_activation'])
    arm = bool(g['cfg_arm'])
    V, B = int(g['cfg_V']), int(g['cfg_B'])
    enc = PerceiverVoxelLangEncoder(
        depth=int(g['cfg_depth']), iterations=1, voxel_size=V, initial_dim=10, low_dim_size=int(g['cfg_low_dim']),
        num_latents=int(g['cfg_latents']), voxel_patch_size=int(g['cfg_k']), voxel_patch_stride=int(g['cfg_s']),
        activation=activation, input_dropout=0.0, attn_dropout=0.0, decoder_dropout=0.0, arm_pred_loss=arm)
    enc.load_state_dict(ow.hashed_state_dict({n: tuple(p.shape) for n, p in enc.named_parameters()}, 0), strict=False)
    enc = enc.to(DEV)
    rs = replay(g, arm)
    eng = enc.engine()
    assert eng.act == ops.ACTIVATIONS[activation]
    eng.precision = precision
    outs, cache = eng.forward(T(g['grid']).to(DEV), rs['low_dim_state'].to(DEV), rs['lang_token_embs'].to(DEV), training=False, save=True)
    errs = [maxerr(outs[0], T(g['q_trans'])), maxerr(outs[1], T(g['rot_grip'])), maxerr(outs[2], T(g['collision']))]
    if arm:
        errs.append(maxerr(outs[3], T(g['arm_out'])))
    print('%s %s forward max-abs %s' % (activation, precision, errs))
    assert max(errs) < TOL_Q, errs
    total, dq, d_o = heads_loss(outs[0], cache['o'], rs['trans_action_indicies'], rs['rot_grip_action_indicies'],
                                rs['ignore_collisions'], B, V)
    d_arm = None
    if arm:
        d_arm = torch.empty_like(outs[3])
        la, _ = ops.ce_rows(outs[3], [(0, 2)], rs['label'].int()[:, :1].to(DEV).contiguous(), d_arm, 1.0 / B)
        total = total + la[:, 0]
    loss = float(total.mean())
    assert abs(loss - float(g['loss'])) < 1e-4, (loss, float(g['loss']))
    if activation == 'relu':
        print('relu subgradient choices flipped to the reference run\'s: %d' % force_relu_kinks(cache, g))
    for p in enc.parameters():
        p.grad = None
    eng.backward(cache, dq, d_o, d_arm)
    check_grads(enc, g)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['f17a_encoder_tiny_relu', 'f17a_encoder_tiny_tanh', 'f17a_encoder_c1_relu', 'f17a_encoder_c1_tanh'])
def test_encoder_fixture(golden, name, precision):
    run_fixture(golden(name), precision)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_encoder_2robots_tanh_fixture(golden, precision):
    g = golden('f17c_encoder_2robots_tiny_tanh')
    V, B = int(g['cfg_V']), int(g['cfg_B'])
    enc = PerceiverVoxelLang2RobotsEncoder(
        depth=int(g['cfg_depth']), iterations=1, voxel_size=V, initial_dim=10, low_dim_size=int(g['cfg_low_dim']),
        num_latents=int(g['cfg_latents']), voxel_patch_size=int(g['cfg_k']), voxel_patch_stride=int(g['cfg_s']),
        activation='tanh', input_dropout=0.0, attn_dropout=0.0, decoder_dropout=0.0)
    enc.load_state_dict(ow.hashed_state_dict({n: tuple(p.shape) for n, p in enc.named_parameters()}, 0), strict=False)
    enc = enc.to(DEV)
    rs = replay(g, False)
    eng = enc.engine()
    eng.precision = precision
    outs, cache = eng.forward(T(g['grid']).to(DEV), rs['low_dim_state'].to(DEV), rs['lang_token_embs'].to(DEV), training=False,
                              save=True, proprio_left=T(g['proprio_left']).to(DEV))
    errs = [maxerr(o, T(g[k])) for o, k in zip(outs, ('q_trans_right', 'rot_grip_right', 'collision_right', 'q_trans_left',
                                                      'rot_grip_left_out', 'collision_left'))]
    print('tanh 2robots %s forward max-abs %s' % (precision, errs))
    assert max(errs) < TOL_Q, errs
    tr, dq_r, do_r = heads_loss(outs[0], cache['o'], rs['trans_action_indicies'], rs['rot_grip_action_indicies'], rs['ignore_collisions'], B, V)
    tl, dq_l, do_l = heads_loss(outs[3], cache['left']['o'], T(g['trans_left']), T(g['rot_grip_left']), rs['ignore_collisions'], B, V)
    loss = float((tr + tl).mean())
    assert abs(loss - float(g['loss'])) < 1e-4, (loss, float(g['loss']))
    for p in enc.parameters():
        p.grad = None
    eng.backward(cache, dq_r, do_r, dq_trans_left=dq_l, d_o_left=do_l)
    check_grads(enc, g)


# ------------------------------------------------------------------------------------------------ kernel modes vs float64 PyTorch
def _act64(x, code, slope):
    x = x.double()
    if code == ops.ACT_TANH:
        return torch.tanh(x)
    return torch.where(x > 0, x, x * slope)


def _dact64(d, y, code, slope):
    d, y = d.double(), y.double()
    if code == ops.ACT_TANH:
        return d * (1 - y * y)
    return torch.where(y > 0, d, d * slope)


def _rel(a, ref):
    return float((a.double().cpu() - ref.cpu()).abs().max()) / max(1e-30, float(ref.abs().max()))


ACTS = [(ops.ACT_TANH, 0.0), (ops.ACT_LRELU, 0.0)]


@pytest.fixture
def bf16x3():
    """the halo-conv kernels run in the matrix-core precisions (the engine sets ops.PRECISION per call; its default is 'bf16x3')"""
    old, ops.PRECISION = ops.PRECISION, 'bf16x3'
    yield
    ops.PRECISION = old


@pytest.mark.parametrize('act', [(ops.ACT_TANH, 0.0)])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_linear_epilogues(act, precision):
    """naive, matrix-core and bf16 GEMMs (ops.linear picks by size and mode) with the tanh epilogue"""
    torch.manual_seed(0)
    old, ops.PRECISION = ops.PRECISION, precision
    try:
        for M, N, K in ((3, 64, 4), (96, 64, 256), (512, 256, 512)):
            x = torch.randn(M, K, device=DEV)
            W = torch.randn(N, K, device=DEV) / K ** 0.5
            b = torch.randn(N, device=DEV) * 0.1
            ref = _act64(x.double() @ W.double().t() + b.double(), *act)
            out = ops.linear(x, W, b, act)
            assert _rel(out, ref) < (1e-5 if precision == 'fp32' else 3e-5), (M, N, K, _rel(out, ref))   # (the GEMM's fp32 sums over K)
    finally:
        ops.PRECISION = old


def _conv_ref(x, w, b, pad=1):
    """channels-last x [B,S,S,S,C], replicate padding, w [Cout][Cin][3][3][3] -> float64 channels-last"""
    xp = torch.nn.functional.pad(x.double().permute(0, 4, 1, 2, 3), (pad,) * 6, mode='replicate')
    return torch.nn.functional.conv3d(xp, w.double(), b.double()).permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize('S', [50, 16])
def test_conv3_ss3d_fwd_tanh(S, bf16x3):
    """`final`'s forward (the halo conv fused with the spatial softmax; Winograd on even grids) with the tanh epilogue; V = 50 reaches
    the part-tile edges"""
    torch.manual_seed(1)
    B = 1
    d0 = torch.randn(B, S, S, S, 64, device=DEV)
    u0 = torch.randn(B, S, S, S, 64, device=DEV)
    w = torch.randn(64, 128, 3, 3, 3, device=DEV) * 0.02
    b = torch.randn(64, device=DEV) * 0.1
    u, _ = ops.conv3_ss3d_fwd(d0, u0, ops.conv_weight_fwd(w), b, B, S, act=(ops.ACT_TANH, 0.0))
    pre, _ = ops.conv3_ss3d_fwd(d0, u0, ops.conv_weight_fwd(w), b, B, S, act=ops.ACT_NONE)
    # the epilogue: tanh of the same sums to ~1 ulp; the sums themselves: the bf16x3 (Winograd) conv's accuracy
    assert float((u.double() - torch.tanh(pre.double())).abs().max()) < 3e-7
    ref = torch.tanh(_conv_ref(torch.cat([d0, u0], -1), w, b))
    assert _rel(u, ref) < 1e-4, _rel(u, ref)


def test_pointwise_fwd_tanh():
    torch.manual_seed(2)
    B, S = 1, 50
    x = torch.randn(B, S, S, S, 10, device=DEV)
    W = torch.randn(64, 10, device=DEV) * 0.3
    b = torch.randn(64, device=DEV) * 0.1
    ref = torch.tanh(x.double() @ W.double().t() + b.double())
    y = ops.pointwise_fwd(x, W, b, act=(ops.ACT_TANH, 0.0))
    assert _rel(y, ref) < 1e-6
    y2, _ = ops.pointwise_ss3d_fwd(x, W, b, B, S, act=(ops.ACT_TANH, 0.0))
    assert torch.equal(y, y2)


@pytest.mark.parametrize('act', ACTS)
def test_lrelu_bwd_and_fold_pad_act(act):
    torch.manual_seed(3)
    n = 1 << 16
    y = _act64(torch.randn(n, device=DEV), *act).float()
    dy = torch.randn(n, device=DEV)
    ref = _dact64(dy, y, *act)
    got = ops.lrelu_bwd_(dy.clone(), y, act=act)
    assert _rel(got, ref) < 1e-6
    # fold_pad with the producer's derivative: padded [B, S+2, ...] -> [B, S, ...]
    B, S, C = 1, 50, 64
    src = torch.randn(B, S + 2, S + 2, S + 2, C, device=DEV)
    yv = _act64(torch.randn(B, S, S, S, C, device=DEV), *act).float()
    dst = torch.empty(B, S, S, S, C, device=DEV)
    ops.fold_pad(src, S + 2, C, 0, dst, B, S, C, 1, lrelu_of=yv, act=act)
    plain = torch.empty_like(dst)
    ops.fold_pad(src, S + 2, C, 0, plain, B, S, C, 1)
    assert _rel(dst, _dact64(plain, yv, *act)) < 1e-6


@pytest.mark.parametrize('act', ACTS)
def test_conv3_dgrad_fold_act(act, bf16x3):
    """`final`'s data gradient fused with the padding adjoint and the producer's derivative: the single bf16x3 launch over both column
    blocks (the fp16 leaf / fp16x2 paths: test_conv3_dgrad_fold_fp16_paths_act)"""
    torch.manual_seed(4)
    B, S = 1, 50
    du = torch.randn(B, S, S, S, 64, device=DEV)
    w = torch.randn(64, 128, 3, 3, 3, device=DEV) * 0.02
    y0 = _act64(torch.randn(B, S, S, S, 64, device=DEV), *act).float()
    y1 = _act64(torch.randn(B, S, S, S, 64, device=DEV), *act).float()
    # reference: the data gradient of the replicate-padded conv, float64
    x = torch.zeros(B, S, S, S, 128, device=DEV, dtype=torch.float64, requires_grad=True)
    _conv_ref(x, w, torch.zeros(64, device=DEV)).backward(du.double())
    g = x.grad
    d0 = torch.empty(B, S, S, S, 64, device=DEV)
    d1 = torch.empty(B, S, S, S, 64, device=DEV)
    ops.conv3_dgrad_fold(du, ops.conv_weight_dgrad(w), B, S, 128, [(d0, False, y0), (d1, False, y1)], act=act)
    assert _rel(d0, _dact64(g[..., :64], y0, *act)) < 5e-4
    assert _rel(d1, _dact64(g[..., 64:], y1, *act)) < 5e-4


@pytest.mark.parametrize('act', ACTS)
def test_c1_dgrad_and_pointwise_wgrad_act(act):
    torch.manual_seed(5)
    B, S = 1, 48
    u = _act64(torch.randn(B, S, S, S, 64, device=DEV), *act).float()
    dq = torch.randn(B, S, S, S, device=DEV)
    w = torch.randn(1, 64, 3, 3, 3, device=DEV) * 0.1
    x = torch.zeros(B, S, S, S, 64, device=DEV, dtype=torch.float64, requires_grad=True)
    _conv_ref(x, w, torch.zeros(1, device=DEV)).backward(dq.double().unsqueeze(-1))
    du = torch.empty(B, S, S, S, 64, device=DEV)
    ops.conv3_c1_dgrad(dq, w, u, du, B, S, accumulate=False, mask=True, act=act)
    assert _rel(du, _dact64(x.grad, u, *act)) < 1e-5
    # the input conv's parameter gradients from dy * act'(y)
    xin = torch.randn(B, S, S, S, 10, device=DEV)
    dy = torch.randn(B, S, S, S, 64, device=DEV)
    dW = torch.zeros(64, 10, device=DEV)
    db = torch.zeros(64, device=DEV)
    ops.pointwise_wgrad(xin, u, dy, dW, db, act=act)
    dpre = _dact64(dy, u, *act).reshape(-1, 64)
    assert _rel(dW, dpre.t() @ xin.double().reshape(-1, 10)) < 1e-5
    assert _rel(db, dpre.sum(0)) < 1e-5


def test_act_code_3_is_refused():
    from voxactb_amd import _lib
    x = torch.zeros(64, 64, device=DEV)
    with pytest.raises(_lib.VoxactbHipError):
        ops.linear(x, x, None, (3, 0.0))
    with pytest.raises(_lib.VoxactbHipError):
        ops.lrelu_bwd_(x, x, act=(3, 0.0))


# ------------------------------------------------------------------------------------------------ agent level
def make_agent(activation):
    cfg = lu.default_cfg(method__voxel_sizes=[16], method__voxel_patch_size=3, method__voxel_patch_stride=4,
                         method__transformer_depth=2, method__num_latents=32, replay__batch_size=2, method__input_dropout=0.0,
                         method__attn_dropout=0.0, method__activation=activation, rlbench__cameras=['front', 'wrist'],
                         rlbench__camera_resolution=[16, 16])
    cfg.method.transform_augmentation.apply_se3 = False
    agent = lu.create_agent(cfg)
    enc = agent._pose_agent._qattention_agents[0]._perceiver_encoder
    assert enc.activation == activation
    enc.load_state_dict(ow.hashed_state_dict({n: tuple(p.shape) for n, p in enc.named_parameters()}, 0), strict=False)
    agent.build(training=True, device=0)
    return agent


def raw_batch(seed):
    rs = synthetic.make_replay_sample(2, ['front', 'wrist'], (16, 16), 16, 4, seed=seed)
    return {k: v.to(DEV) for k, v in rs.items()}


@pytest.mark.parametrize('activation', ['relu', 'tanh'])
def test_agent_updates_act_and_weights(activation, tmp_path):
    agent = make_agent(activation)
    batch = raw_batch(10)
    losses = [float(agent.update(step, batch)['total_losses']) for step in range(10)]
    print(activation, losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    enc = agent._pose_agent._qattention_agents[0]._perceiver_encoder
    agent.save_weights(str(tmp_path))
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    for p in enc.parameters():
        p.data.add_(1.0)
    agent.load_weights(str(tmp_path))
    assert all(torch.equal(before[n], p.detach()) for n, p in enc.named_parameters())
    rs = synthetic.make_replay_sample(1, ['front', 'wrist'], (16, 16), 16, 4, seed=3)
    obs = {k: v.to(DEV) for k, v in rs.items()
           if k.endswith(('_rgb', '_point_cloud', '_camera_extrinsics', '_camera_intrinsics')) or k == 'low_dim_state'}
    obs = {k: v.unsqueeze(0) if v.dim() < 5 and k.endswith(('_rgb', '_point_cloud')) else v for k, v in obs.items()}
    for cam in ('front', 'wrist'):
        obs['%s_camera_extrinsics' % cam][0, 0, 2, 3] = -1.0
    obs['low_dim_state'] = rs['low_dim_state'].to(DEV)
    obs['lang_goal_emb'] = rs['lang_goal_emb'][0].to(DEV)
    obs['lang_token_embs'] = rs['lang_token_embs'][0].to(DEV)
    res = agent.act(0, obs, deterministic=True)
    assert res.action.shape == (9,) and np.isfinite(res.action).all()


def test_interleaved_engines_keep_their_activation():
    """an lrelu agent stepped alone, and again interleaved step by step with a tanh agent in the same process: the same bits"""
    batch = raw_batch(12)

    def steps(with_other):
        torch.manual_seed(0)
        a = make_agent('lrelu')
        b = make_agent('tanh') if with_other else None
        out = []
        for step in range(3):
            out.append(float(a.update(step, batch)['total_losses']))
            if b is not None:
                b.update(step, batch)
        enc = a._pose_agent._qattention_agents[0]._perceiver_encoder
        return out, [p.detach().clone() for p in enc.parameters()]

    la, pa = steps(False)
    lb, pb = steps(True)
    assert la == lb
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('S', [50, 49])
def test_conv3_dgrad_fold_fp16_paths_act(act, S, bf16x3):
    """the default training step's form of the same data gradient (WGRAD_PRECISION 'fp16', engine defaults): block 0 a leaf on one fp16
    product, block 1 on two fp16 products (Winograd on even grids, direct on odd ones) with its own operand scale taken in the epilogue
    after the derivative"""
    torch.manual_seed(6)
    B = 1
    du = torch.randn(B, S, S, S, 64, device=DEV)
    w = torch.randn(64, 128, 3, 3, 3, device=DEV) * 0.02
    y0 = _act64(torch.randn(B, S, S, S, 64, device=DEV), *act).float()
    y1 = _act64(torch.randn(B, S, S, S, 64, device=DEV), *act).float()
    x = torch.zeros(B, S, S, S, 128, device=DEV, dtype=torch.float64, requires_grad=True)
    _conv_ref(x, w, torch.zeros(64, device=DEV)).backward(du.double())
    g = x.grad
    d0 = torch.empty(B, S, S, S, 64, device=DEV)
    d1 = torch.empty(B, S, S, S, 64, device=DEV)
    old = ops.WGRAD_PRECISION, ops.DGRAD_PRECISION
    ops.WGRAD_PRECISION, ops.DGRAD_PRECISION = 'fp16', 'fp16x2'
    try:
        sc = ops.conv3_dgrad_fold(du, ops.conv_weight_dgrad(w), B, S, 128, [(d0, False, y0), (d1, False, y1)], leaf_blocks=(0,),
                                  scale_blocks=(1,), act=act)
    finally:
        ops.WGRAD_PRECISION, ops.DGRAD_PRECISION = old
    assert _rel(d0, _dact64(g[..., :64], y0, *act)) < 3e-3           # one fp16 product per term
    assert _rel(d1, _dact64(g[..., 64:], y1, *act)) < 5e-4
    assert torch.equal(sc[1], ops.absmax_scale(d1))                   # the scale of what was written, derivative included


def _patch_ref(dpatch, Wp, d0, vox, k, pad, act):
    """float64: d(d0) of the patchify conv (stride k, replicate padding), times act'(d0), into the input conv's dW [64][10] / db [64]"""
    B, V = d0.shape[0], d0.shape[1]
    x = d0.double().permute(0, 4, 1, 2, 3).detach().requires_grad_(True)
    out = torch.nn.functional.conv3d(torch.nn.functional.pad(x, (pad,) * 6, mode='replicate'), Wp.double(), stride=k)
    G = out.shape[-1]
    out.backward(dpatch.double().view(B, G, G, G, 64).permute(0, 4, 1, 2, 3))
    dpre = _dact64(x.grad.permute(0, 2, 3, 4, 1), d0, *act).reshape(-1, 64)
    return dpre.t() @ vox.double().reshape(-1, 10), dpre.sum(0), G


@pytest.mark.parametrize('act', ACTS + [ops.LRELU])
def test_patch_dgrad_input_wgrad_act(act):
    """the fused patchify data gradient -> input conv weight gradient (patch_wgrad.hip; the engine takes it when k == s, the headline's
    5 / 5) with the tanh and the slope-0 derivative, against float64; V = 50 leaves partial edge patches"""
    torch.manual_seed(7)
    B, V, k, pad = 1, 50, 5, 2
    d0 = _act64(torch.randn(B, V, V, V, 64, device=DEV), *act).float().contiguous()
    vox = torch.randn(B, V, V, V, 10, device=DEV)
    Wp = torch.randn(64, 64, k, k, k, device=DEV) * 0.02
    G = (V + 2 * pad - k) // k + 1
    dpatch = torch.randn(B, G ** 3, 64, device=DEV)
    rW, rb, G2 = _patch_ref(dpatch, Wp, d0, vox, k, pad, act)
    assert G2 == G
    dW = torch.zeros(64, 10, device=DEV)
    db = torch.zeros(64, device=DEV)
    ops.patch_dgrad_input_wgrad(dpatch, Wp, d0, vox, dW, db, B, V, G, k, pad, act=act)
    assert _rel(dW, rW) < 3e-3 and _rel(db, rb) < 3e-3, (_rel(dW, rW), _rel(db, rb))      # single fp16 products (a leaf)


@pytest.mark.parametrize('act', ACTS)
def test_fused_ss3d_backward_entries_act(act):
    """the fused backward of u (c1 data gradient + pooled-feature term + derivative + bias sums) and the fused input-conv weight gradient
    with the pooled-feature term, both with zero pooled-feature gradients: they must equal the plain entries (checked against float64
    above) under the new codes"""
    torch.manual_seed(8)
    B, S = 1, 48
    u = _act64(torch.randn(B, S, S, S, 64, device=DEV), *act).float()
    dq = torch.randn(B, S, S, S, device=DEV)
    w = torch.randn(1, 64, 3, 3, 3, device=DEV) * 0.1
    ss, mx, st, am = ops.ss3d_max_fwd(u, S ** 3 * 64, B, S, 64)
    g_ss, g_max = torch.zeros_like(ss), torch.zeros_like(mx)
    du = torch.empty_like(u)
    dbias = torch.zeros(64, device=DEV)
    ops.conv3_c1_dgrad_ss3d(dq, w, u, du, B, S, st, ss, am, g_ss, g_max, dbias, act=act)
    ref = torch.empty_like(u)
    ops.conv3_c1_dgrad(dq, w, u, ref, B, S, accumulate=False, mask=True, act=act)
    assert _rel(du, ref.double()) < 1e-6
    assert _rel(dbias, ref.double().reshape(-1, 64).sum(0)) < 1e-5
    xin = torch.randn(B, S, S, S, 10, device=DEV)
    dy = torch.randn(B, S, S, S, 64, device=DEV)
    dW, db = torch.zeros(64, 10, device=DEV), torch.zeros(64, device=DEV)
    ops.pointwise_wgrad_ss3d(xin, u, dy, dW, db, B, S, st, ss, am, g_ss, g_max, act=act)
    dpre = _dact64(dy, u, *act).reshape(-1, 64)
    assert _rel(dW, dpre.t() @ xin.double().reshape(-1, 10)) < 1e-5
    assert _rel(db, dpre.sum(0)) < 1e-5


@pytest.mark.parametrize('wide_dispatch', [True], indirect=True)
def test_wide_gemm_tanh_epilogue(wide_dispatch, bf16x3):
    """the 128 x 512-tile GEMM the B = 16 step dispatches for the dense layers (from 1024 rows here, conftest.wide_dispatch): the tanh
    epilogue against tanh of the same kernel's sums, and against float64"""
    torch.manual_seed(9)
    x = torch.randn(2048, 512, device=DEV)
    W = torch.randn(512, 512, device=DEV) / 512 ** 0.5
    b = torch.randn(512, device=DEV) * 0.1
    out = ops.linear(x, W, b, (ops.ACT_TANH, 0.0))
    pre = ops.linear(x, W, b, ops.ACT_NONE)
    assert float((out.double() - torch.tanh(pre.double())).abs().max()) < 3e-7
    assert _rel(out, torch.tanh(x.double() @ W.double().t() + b.double())) < 3e-5


# ------------------------------------------------------------------------------------------------ headline geometry (F17b)
def _c2_setup(g):
    from voxactb_amd.voxel.voxel_grid import VoxelGrid
    V, B, H, W = int(g['cfg_V']), int(g['cfg_B']), int(g['cfg_H']), int(g['cfg_W'])
    cams = [str(c) for c in g['cfg_cams']]
    enc = PerceiverVoxelLangEncoder(
        depth=int(g['cfg_depth']), iterations=1, voxel_size=V, initial_dim=10, low_dim_size=int(g['cfg_low_dim']),
        num_latents=int(g['cfg_latents']), voxel_patch_size=int(g['cfg_k']), voxel_patch_stride=int(g['cfg_s']),
        activation=str(g['cfg_activation']), input_dropout=0.0, attn_dropout=0.0, decoder_dropout=0.0)
    enc.load_state_dict(ow.hashed_state_dict({n: tuple(p.shape) for n, p in enc.named_parameters()}, 0), strict=False)
    enc = enc.to(DEV)
    rs = replay(g, False)
    vg = VoxelGrid(synthetic.SCENE_BOUNDS, V, DEV, B, 3, H * W * len(cams))
    grid = vg.voxelize_cameras([rs['%s_point_cloud' % c].to(DEV) for c in cams], [rs['%s_rgb' % c].to(DEV) for c in cams],
                               torch.tensor([synthetic.SCENE_BOUNDS]).to(DEV))
    return enc, rs, grid, V, B


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('activation', ['relu', 'tanh'])
def test_encoder_headline_fixture(golden, activation, precision):
    """F17b: V = 100, depth 6, 2048 latents, B = 1 -- the step's headline kernels (Winograd `final` fused with the spatial softmax,
    polyphase up-conv, fused patchify weight gradient (k == s), fp16 weight / fp16x2 data gradients, fused backward of u).  The gates of
    tests/test_c2_reference_gpu.py: occupancy bit-exact, Q digest / heads within 1e-4, loss within 1e-4, every gradient norm within 3e-3
    (conv biases: against the float64 sums of the reference's dY), small gradients element-wise -- the backward at the reference run's
    max-pool choices (and, for relu, subgradient choices) where those are ties."""
    from tests.test_c2_reference_gpu import _check_grid, _check_forward, force_pools
    g = golden('f17b_encoder_c2_%s' % activation)
    enc, rs, grid, V, B = _c2_setup(g)
    _check_grid(g, grid)
    eng = enc.engine()
    eng.precision = precision
    outs, cache = eng.forward(grid, rs['low_dim_state'].to(DEV), rs['lang_token_embs'].to(DEV), training=False, save=True,
                              lang_goal_emb=rs['lang_goal_emb'].to(DEV))
    _check_forward(g, outs, False, '%s/%s' % (activation, precision))
    total, dq, d_o = heads_loss(outs[0], cache['o'], rs['trans_action_indicies'], rs['rot_grip_action_indicies'],
                                rs['ignore_collisions'], B, V)
    loss = float(total.mean())
    assert abs(loss - float(g['loss'])) < 1e-4, (loss, float(g['loss']))
    if activation == 'relu':
        print('relu subgradient choices flipped to the reference run\'s: %d' % force_relu_kinks(cache, g))
    print('max-pool ties flipped to the reference run\'s: %s' % force_pools(cache, g, eng.T0))
    for p in enc.parameters():
        p.grad = None
    eng.backward(cache, dq, d_o, None)
    P = dict(enc.named_parameters())
    bad = []
    for n, rn in zip([str(n) for n in g['grad_names']], T(g['grad_norms'])):
        key64 = 'dysum64__' + n
        if key64 in g.files:        # a conv bias: a sum over 10^6 voxels, against the float64 sum of the reference's dY (F5g's gate)
            ref = T(g[key64])
            e = float((P[n].grad.double().cpu() - ref).abs().max())
            if e > 2e-3 * float(ref.abs().max()) + 2e-5:
                bad.append((n, 'vs float64 dY sum', e, float(ref.abs().max())))
            continue
        gn, rn = float(P[n].grad.norm()), float(rn)
        if abs(gn - rn) > GRAD_TOL * rn + 1e-5:
            bad.append((n, gn, rn))
        key = 'grad__' + n
        if key in g.files:
            ref = T(g[key])
            e = maxerr(P[n].grad, ref)
            if e > GRAD_TOL * float(ref.abs().max()) + 1e-5:
                bad.append((n, 'full', e, float(ref.abs().max())))
    assert not bad, bad
    del cache, outs
    torch.cuda.empty_cache()
