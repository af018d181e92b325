#!/usr/bin/env python
"""Generate the F17 fixtures (tests/golden/f17*.npz): the REFERENCE encoder built with activation='relu' or 'tanh'.

Same recipe as make_golden.py (whose helpers this imports; it stays untouched): hashed weights, dropout 0, the synthetic batch of
seed 1, the loss the product tests differentiate.  oracle/ is LeakyReLU-only, so these fixtures pin the new activations directly.

    python tests/golden/make_golden_activation.py [--only f17a,f17b,f17c]

F17a: CFG_TINY (arm_pred_loss) and CFG_C1 -- full forward outputs, every parameter gradient's norm (the small ones in full), and the
      reference run's pre-activations within KINK_TAU of zero at the grid-sized blocks (ReLU' jumps there).
F17b: CFG_C2, the headline geometry (V = 100, depth 6, B = 1), relu and tanh -- only at 10^6 voxels does the product take its
      headline kernels (Winograd `final`, polyphase up-conv, the fused patchify weight gradient, fp16 weight gradients, the fused
      spatial-softmax paths): forward digest, loss, gradient norms, float64 sums of the conv-bias dY, pool and (relu) kink data.
F17c: the 2Robots encoder (one_policy_more_heads) at CFG_TINY with tanh: it reaches the dense*_left_arm blocks.
Reference forward + backward time on a CPU (this generator's last run): F17a tiny relu 0.4 s, tanh < 0.1 s; C1 relu 0.5 s, tanh 0.4 s;
F17b relu and tanh about 15 s each; F17c < 0.1 s.
"""
import argparse
import os
import sys
import time

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402
from make_golden import ow, ovox, oagent, synthetic  # noqa: E402


def make_ref_encoder(cfg, activation, arm=False, two_robots=False):
    cls = mg.ref_pl.PerceiverVoxelLang2RobotsEncoder if two_robots else mg.ref_pl.PerceiverVoxelLangEncoder
    kw = {} if two_robots else dict(arm_pred_loss=arm)
    enc = cls(depth=cfg['depth'], iterations=1, voxel_size=cfg['V'], initial_dim=10, low_dim_size=cfg['low_dim'],
              num_latents=cfg['latents'], voxel_patch_size=cfg['k'], voxel_patch_stride=cfg['s'], activation=activation,
              input_dropout=0.0, attn_dropout=0.0, decoder_dropout=0.0, **kw)
    shapes = {n: tuple(p.shape) for n, p in enc.named_parameters()}
    enc.load_state_dict(ow.hashed_state_dict(shapes, 0), strict=False)
    return enc.eval()


def grid_for(cfg, rs):
    pcd = [rs['%s_point_cloud' % c] for c in cfg['cams']]
    rgb = [rs['%s_rgb' % c] for c in cfg['cams']]
    bounds = torch.tensor([synthetic.SCENE_BOUNDS])
    coords, feats = ovox.flatten_cameras(pcd, rgb)
    return mg.ref_voxelize(coords, feats, bounds, cfg['V'], cfg['B']), bounds


def cfg_arrays(cfg, activation, arm):
    return dict(cfg_V=cfg['V'], cfg_k=cfg['k'], cfg_s=cfg['s'], cfg_depth=cfg['depth'], cfg_latents=cfg['latents'],
                cfg_low_dim=cfg['low_dim'], cfg_B=cfg['B'], cfg_H=cfg['H'], cfg_W=cfg['W'], cfg_cams=np.array(cfg['cams']),
                cfg_arm=int(arm), cfg_activation=np.array(activation))


def grads(enc, arrs):
    arrs['grad_names'] = np.array([n for n, _ in enc.named_parameters()])
    arrs['grad_norms'] = torch.stack([p.grad.norm() for _, p in enc.named_parameters()])
    for n, p in enc.named_parameters():
        if p.numel() <= 20000 and not n.startswith(('pos_encoding', 'latents')):
            arrs['grad__' + n] = p.grad


def f17a(name, cfg, activation, arm=False):
    enc = make_ref_encoder(cfg, activation, arm)
    rs = mg.batch_for(cfg, seed=1, arm=arm)
    grid, bounds = grid_for(cfg, rs)
    kinks = {}
    hooks = mg.capture_kinks(enc, kinks)
    t0 = time.time()
    outs = enc(grid.permute(0, 4, 1, 2, 3), rs['low_dim_state'], rs['lang_goal_emb'], rs['lang_token_embs'], None, bounds, None)
    total, _ = oagent.losses(outs[0], outs[1], outs[2], rs['trans_action_indicies'], rs['rot_grip_action_indicies'],
                             rs['ignore_collisions'], outs[3] if arm else None, rs.get('label'))
    total.backward()
    print('%s: reference forward + backward %.1fs, loss %.6f' % (name, time.time() - t0, float(total.detach())))
    for h in hooks:
        h.remove()
    arrs = cfg_arrays(cfg, activation, arm)
    arrs.update(grid=grid, q_trans=outs[0].detach(), rot_grip=outs[1].detach(), collision=outs[2].detach(), loss=total.detach())
    if arm:
        arrs['arm_out'] = outs[3].detach()
    grads(enc, arrs)
    if activation == 'relu':
        arrs.update(kinks, kink_tau=mg.KINK_TAU)
        print('%s: pre-activations within %.0e of zero: %s' % (name, mg.KINK_TAU, {k.split('__')[1]: int(v.numel()) for k, v in kinks.items() if k.endswith('idx')}))
    mg.save(name, **arrs)


def f17b(name, cfg, activation):
    """headline geometry (CFG_C2: V = 100, depth 6, 2048 latents, B = 1): a digest of the forward (as F5: the 10^6 Q-values are not
    stored), the loss, every gradient's norm (small ones in full), the arg-max / top-2 margin of the three global max pools (as
    make_golden.pool_choices) and, for relu, the pre-activations within KINK_TAU of zero.  The grid is not stored either: its occupancy
    and channel sums are, and the test voxelizes the same seeded clouds on the device."""
    enc = make_ref_encoder(cfg, activation)
    rs = mg.batch_for(cfg, seed=1)
    grid, bounds = grid_for(cfg, rs)
    kinks, pools, dy_sums = {}, [], {}
    hooks = mg.capture_kinks(enc, kinks) if activation == 'relu' else []
    hooks.append(mg._pool_hook(enc, pools))

    def tap(nm):        # conv-bias gradients sum dY over 10^6 voxels: the float64 sums of the same dY next to the fp32 ones (as F5g)
        def fwd_hook(mod, inp, out):
            out.register_hook(lambda gr: dy_sums.__setitem__(nm, gr.double().sum(dim=(0, 2, 3, 4))))
        return fwd_hook
    for n, m_ in enc.named_modules():
        if isinstance(m_, torch.nn.Conv3d):
            hooks.append(m_.register_forward_hook(tap(n)))
    t0 = time.time()
    outs = enc(grid.permute(0, 4, 1, 2, 3), rs['low_dim_state'], rs['lang_goal_emb'], rs['lang_token_embs'], None, bounds, None)
    total, _ = oagent.losses(outs[0], outs[1], outs[2], rs['trans_action_indicies'], rs['rot_grip_action_indicies'],
                             rs['ignore_collisions'])
    total.backward()
    print('%s: reference forward + backward %.1fs, loss %.6f' % (name, time.time() - t0, float(total.detach())))
    for h in hooks:
        h.remove()
    assert len(pools) == 3
    arrs = cfg_arrays(cfg, activation, False)
    flat = outs[0].detach().reshape(cfg['B'], -1)
    top = flat.topk(16, dim=1)
    sidx = ow.hashed_int('digest', (4096,), 0, flat.shape[1])
    occ = grid[..., -1] > 0
    arrs.update(q_trans_argmax=flat.argmax(1), q_trans_top_vals=top.values, q_trans_top_idx=top.indices, q_trans_sample_idx=sidx,
                q_trans_sample=flat[:, sidx], q_trans_lse=torch.logsumexp(flat.double(), 1), grid_occ_count=occ.sum(), grid_occ_flat=torch.nonzero(occ.reshape(-1))[:, 0].int(),
                grid_channel_sums=grid.double().sum(dim=(0, 1, 2, 3)), rot_grip=outs[1].detach(), collision=outs[2].detach(),
                loss=total.detach())
    for i, (am, mg_) in enumerate(pools):
        arrs['pool_argmax_%d' % i] = am
        arrs['pool_margin_%d' % i] = mg_
    grads(enc, arrs)
    for n, v in dy_sums.items():
        arrs['dysum64__' + n + '.bias'] = v
    if activation == 'relu':
        arrs.update(kinks, kink_tau=mg.KINK_TAU)
        print('%s: pre-activations within %.0e of zero: %s' % (name, mg.KINK_TAU, {k.split('__')[1]: int(v.numel()) for k, v in kinks.items() if k.endswith('idx')}))
    mg.save(name, **arrs)


def f17c(name, cfg, activation):
    enc = make_ref_encoder(cfg, activation, two_robots=True)
    rs = mg.batch_for(cfg, seed=1)
    grid, bounds = grid_for(cfg, rs)
    B, V = cfg['B'], cfg['V']
    proprio_left = ow.hashed_uniform('f11.proprio_left', (B, cfg['low_dim']), 0.0, 1.0)
    trans_left = ow.hashed_int('f11.trans_left', (B, 3), 0, V)
    rot_left = torch.cat((ow.hashed_int('f11.rot_left', (B, 3), 0, 72), ow.hashed_int('f11.grip_left', (B, 1), 0, 2)), 1)
    t0 = time.time()
    outs = enc(grid.permute(0, 4, 1, 2, 3), rs['low_dim_state'], proprio_left, rs['lang_goal_emb'], rs['lang_token_embs'], None, bounds, None)
    tr, _ = oagent.losses(outs[0], outs[1], outs[2], rs['trans_action_indicies'], rs['rot_grip_action_indicies'], rs['ignore_collisions'])
    tl, _ = oagent.losses(outs[3], outs[4], outs[5], trans_left, rot_left, rs['ignore_collisions'])
    total = tr + tl
    total.backward()
    print('%s: reference forward + backward %.1fs, loss %.6f' % (name, time.time() - t0, float(total.detach())))
    arrs = cfg_arrays(cfg, activation, False)
    arrs.update(grid=grid, proprio_left=proprio_left, trans_left=trans_left, rot_grip_left=rot_left,
                q_trans_right=outs[0].detach(), rot_grip_right=outs[1].detach(), collision_right=outs[2].detach(),
                q_trans_left=outs[3].detach(), rot_grip_left_out=outs[4].detach(), collision_left=outs[5].detach(), loss=total.detach())
    grads(enc, arrs)
    mg.save(name, **arrs)


SECTIONS = {
    'f17a': lambda: [f17a('f17a_encoder_tiny_%s' % a, mg.CFG_TINY, a, arm=True) for a in ('relu', 'tanh')]
    + [f17a('f17a_encoder_c1_%s' % a, mg.CFG_C1, a) for a in ('relu', 'tanh')],
    'f17b': lambda: [f17b('f17b_encoder_c2_%s' % a, mg.CFG_C2, a) for a in ('relu', 'tanh')],
    'f17c': lambda: f17c('f17c_encoder_2robots_tiny_tanh', mg.CFG_TINY, 'tanh'),
}

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    torch.manual_seed(0)
    for key in (args.only.split(',') if args.only else SECTIONS):
        SECTIONS[key]()
