"""Drop-in replacement for the reference's ``med3d.py`` network factories.

Same surface as reference med3d.py:187-425: ``resnet{18,34,50}seg{cls,reg}(**kwargs)``
return an ``nn.Module`` with ``forward(x, lungs=None) -> (dense_outs, outs)``,
``get_target_layer()``, and a ``state_dict()`` whose keys/shapes are identical to the
reference (``conv1.weight [64,1,7,7,7]`` ... ``fcs.1.bias``), so Hydra ``_target_`` confs,
``load_state_dict_greedy`` and Lightning checkpoints keep working.  Parameters live in
ordinary ``nn.Conv3d`` / ``nn.BatchNorm3d`` *containers* created in the reference's order
(same seed => same initial weights); none of their ``forward`` methods is ever called --
the arithmetic runs in libdram_hip.so through ``engine.Engine``.

There is no CPU path: calling the network on a CPU tensor raises.
"""
from __future__ import annotations

if not __package__:          # imported top-level (this directory on sys.path): bind to the package, see _dropin.py
    import _dropin
    __package__ = _dropin.adopt(__name__)

import os
from typing import List, Optional

import torch
import torch.nn as nn

from . import ops
from .engine import ARCHS, EXPANSION, Engine

__all__ = ["ResNetSegCls", "ResNetSegReg", "resnet18segcls", "resnet34segcls", "resnet50segcls",
           "resnet18segreg", "resnet34segreg", "resnet50segreg", "BasicBlock", "Bottleneck",
           "UpsampleConvBlock5d"]


def _conv3(cin, cout, stride=1, dilation=1):
    return nn.Conv3d(cin, cout, kernel_size=3, dilation=dilation, stride=stride, padding=dilation, bias=False)


class _Container(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container: the fused engine runs the whole network "
                           "(call the ResNetSeg* module instead)")


class BasicBlock(_Container):
    """Parameter layout of reference BasicBlock (med3d.py:115-127)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=False):
        super().__init__()
        self.conv1 = _conv3(inplanes, planes, stride, dilation)
        self.bn1 = nn.BatchNorm3d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _conv3(planes, planes, 1, dilation)
        self.bn2 = nn.BatchNorm3d(planes)
        self.stride, self.dilation, self.has_shortcut_a = stride, dilation, bool(downsample)


class Bottleneck(_Container):
    """Parameter layout of reference Bottleneck (med3d.py:147-162)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=False):
        super().__init__()
        self.conv1 = nn.Conv3d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm3d(planes)
        self.conv2 = nn.Conv3d(planes, planes, kernel_size=3, stride=stride, dilation=dilation, padding=dilation,
                               bias=False)
        self.bn2 = nn.BatchNorm3d(planes)
        self.conv3 = nn.Conv3d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm3d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.stride, self.dilation, self.has_shortcut_a = stride, dilation, bool(downsample)


class UpsampleConvBlock5d(_Container):
    """Parameter layout of reference UpsampleConvBlock5d (med3d.py:50-83), dropout == 0."""

    def __init__(self, in_chs, base_chs):
        super().__init__()
        self.conv_blocks = nn.Sequential(*[
            nn.Sequential(nn.Conv3d(i, o, kernel_size=3, padding=1, bias=True), nn.BatchNorm3d(o), nn.ReLU(inplace=True))
            for i, o in zip(in_chs, base_chs)])
        self.upsample = nn.Upsample(size=None, scale_factor=2, mode="trilinear", align_corners=True)


class _Med3DFunction(torch.autograd.Function):
    """Whole-network autograd node: forward/backward are engine walks over HIP kernels."""

    @staticmethod
    def forward(ctx, module, x, lungs, *params):
        ctx.set_materialize_grads(False)
        P = module._tensor_dict()
        # (x, then the parameters; a partially frozen parameter set computes every parameter gradient, as before)
        need_x, need_param = ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:])
        dense, outs, saved = module._engine.forward(P, x, lungs, module.training, True, module._dist,
                                                    module.activation_recompute, module._storage_now(),
                                                    need_x=need_x, need_param=need_param)
        ctx.saved_state = saved
        ctx.module = module
        return dense[0], dense[1], outs[0], outs[1]

    @staticmethod
    def backward(ctx, gd0, gd1, go0, go1):
        module = ctx.module
        saved, ctx.saved_state = ctx.saved_state, None
        if saved is None:
            raise RuntimeError("backward through the Med3D engine a second time (buffers were freed)")

        def c(t):
            return None if t is None else t.contiguous()

        grads = module._engine.backward(saved, [c(gd0), c(gd1)], [c(go0), c(go1)])
        out = [None, saved.get("dx") if ctx.needs_input_grad[1] else None, None]     # (no gradient for lungs)
        for name, p in module._named_tensors()[0]:
            out.append(grads.get(name) if p.requires_grad else None)
        return tuple(out)


class _ResNetSeg(nn.Module):
    HEAD = None

    def __init__(self, block, layers, shortcut_type="A", n_classes=(6, 3)):
        super().__init__()
        if shortcut_type != "A":
            # the reference's shortcut 'B' (med3d.py:250-257) is not reachable from any conf/*.yaml
            raise NotImplementedError("only shortcut_type='A' (every reference conf) is implemented")
        self.inplanes = 64
        self.conv1 = nn.Conv3d(1, 64, kernel_size=7, stride=(2, 2, 2), padding=(3, 3, 3), bias=False)
        self.bn1 = nn.BatchNorm3d(64)
        self.relu = nn.ReLU(inplace=True)
        self.n_classes = list(n_classes)
        self.maxpool = nn.MaxPool3d(kernel_size=(3, 3, 3), stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=1, dilation=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=1, dilation=4)
        self.us1 = UpsampleConvBlock5d([(512 + 64) * block.expansion, 64], [64, 64])
        self.us2 = UpsampleConvBlock5d([64 + 64, 64], [64, 64])
        self.us3 = nn.Sequential(nn.Conv3d(64, 32, kernel_size=3, padding=1), nn.BatchNorm3d(32), nn.ReLU(inplace=True))
        self.fcs = nn.ModuleList([nn.Conv3d(32, n, kernel_size=1, padding=0, stride=1, bias=True)
                                  for n in self.n_classes])
        for m in self.modules():  # med3d.py:235-240
            if isinstance(m, nn.Conv3d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
            elif isinstance(m, nn.BatchNorm3d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
        kind = "basic" if block is BasicBlock else "bottleneck"
        net = [k for k, v in ARCHS.items() if v == (kind, tuple(layers))]
        if not net:
            raise NotImplementedError(f"layer configuration {layers} has no engine plan")
        assert EXPANSION[kind] == block.expansion
        self._engine = Engine(net[0], self.HEAD)
        self._dist = None  # set by distributed.attach()
        # Activation recompute (the build-side "activation checkpointing" of BASELINE configs[4]; the reference's
        # checkpoint_segments argument is stored and never used, med3d.py:52,56): backward re-derives BN+ReLU
        # outputs inside a block, the upsample+concat tensors and the cached Winograd-domain images instead of
        # keeping them.  Same kernels on the same inputs: gradients are bit-identical, peak HBM drops, the step
        # gets ~7 % longer.  Default from the environment (DRAM_RECOMPUTE=1).
        self.activation_recompute = os.environ.get("DRAM_RECOMPUTE", "0") == "1"
        # Storage type of the activations.  float32 = the reference's default arithmetic.  bfloat16 = what the
        # reference runs under Lightning's `--precision bf16` (train.py:46 -> torch.autocast(bfloat16)): selected
        # automatically inside an autocast(bfloat16) region, or explicitly (module.storage_dtype = torch.bfloat16 /
        # DRAM_STORAGE=bf16).  Parameters, BatchNorm statistics, gradients and the returned tensors stay float32.
        self.storage_dtype = torch.bfloat16 if os.environ.get("DRAM_STORAGE", "f32") == "bf16" else torch.float32

    def _make_layer(self, block, planes, blocks, stride=1, dilation=1):
        ds = stride != 1 or self.inplanes != planes * block.expansion  # med3d.py:244
        layers = [block(self.inplanes, planes, stride=stride, dilation=dilation, downsample=ds)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, dilation=dilation))
        return nn.Sequential(*layers)

    def get_target_layer(self):
        return self.us3

    def _storage_now(self):
        if torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() == torch.bfloat16:
            return torch.bfloat16
        return self.storage_dtype

    def _named_tensors(self):
        """(named_parameters(), named_buffers()) as lists, in nn.Module's own order, without nn.Module's recursive
        generators: three such traversals per step were 1.5 ms of a ResNet-50 step's 15 ms of host time.  The list of
        submodules is taken once (the constructor builds all of them); parameters and buffers are read from the
        submodules' own dicts every time, so `.to()` / `load_state_dict` / a replaced tensor are always seen."""
        mods = self.__dict__.get("_submodules")
        if mods is None:
            mods = self.__dict__["_submodules"] = [((pre + ".") if pre else "", m) for pre, m in self.named_modules()]
        params, bufs = [], []
        for pre, m in mods:
            for k, p in m._parameters.items():
                if p is not None:
                    params.append((pre + k, p))
            for k, b in m._buffers.items():
                if b is not None:
                    bufs.append((pre + k, b))
        return params, bufs

    def _tensor_dict(self):
        params, bufs = self._named_tensors()
        d = dict(params)
        d.update(bufs)
        return d

    def _check_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("bodyct-dram-emph-subtype_amd runs on MI355X only: input is on "
                               f"{x.device}; there is no CPU fallback (the CPU oracle lives in oracle/ for tests)")
        if x.dim() != 5 or x.shape[1] != 1:
            raise ValueError(f"expected x of shape [B,1,D,H,W], got {tuple(x.shape)}")
        if any(int(s) % 8 for s in x.shape[-3:]):
            # crop_concat_5d (med3d.py:39-48) mis-crops otherwise; the reference only asserts on W
            raise ValueError("input D,H,W must be multiples of 8")

    def forward(self, x: torch.Tensor, lungs: Optional[torch.Tensor] = None):
        """-> (dense_outs, outs).  Differentiable with respect to the parameters and to x (`x.requires_grad_()`; not to
        lungs), in train() and in eval() mode -- eval: BatchNorm on its running statistics in both directions, no
        buffer touched.  When no parameter requires a gradient, backward runs the data-gradient chain only."""
        self._check_input(x)
        x = x.contiguous().float()
        if lungs is not None:
            lungs = lungs.contiguous().float()
        params = [p for _, p in self._named_tensors()[0]]
        need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        if need_grad:
            d0, d1, o0, o1 = _Med3DFunction.apply(self, x, lungs, *params)
            return [d0, d1], [o0, o1]
        with torch.no_grad():
            dense, outs, _ = self._engine.forward(self._tensor_dict(), x, lungs, self.training, False, self._dist,
                                                  storage=self._storage_now())
        return dense, outs

    def input_gradient(self, x: torch.Tensor, lungs: Optional[torch.Tensor] = None, *, out_grads,
                       dense_grads=None) -> torch.Tensor:
        """Gradient of a score with respect to the volume: runs forward(x, lungs) in the module's current mode
        (eval(): running statistics, nothing updated; train(): a training forward, running statistics included) and
        backward from the given cotangents -- out_grads = (g0, g1) for `outs`, dense_grads = (g0, g1) for `dense_outs`,
        each a tensor shaped like its output or None -- along the data-gradient chain only: no weight-gradient kernel
        runs and no parameter's .grad is touched.  Returns [B,1,D,H,W] float32, bit-identical to x.grad of the
        `x.requires_grad_()` + backward() route.  Under distributed.attach the result is local to the rank."""
        self._check_input(x)
        x = x.detach().contiguous().float()
        if lungs is not None:
            lungs = lungs.detach().contiguous().float()

        def pair(gs, name):
            gs = [None, None] if gs is None else list(gs)
            if len(gs) != 2:
                raise ValueError(f"{name}: expected two cotangents (or None), got {len(gs)}")
            return gs

        og, dg = pair(out_grads, "out_grads"), pair(dense_grads, "dense_grads")
        if all(g is None for g in og + dg):
            raise ValueError("input_gradient: every cotangent is None")
        for gs, name in ((og, "out_grads"), (dg, "dense_grads")):      # before anything is launched (or updated)
            for i, g in enumerate(gs):
                if g is not None and (not isinstance(g, torch.Tensor) or g.device != x.device):
                    raise ValueError(f"{name}[{i}]: expected a tensor on {x.device} (or None)")
        with torch.no_grad():
            dense, outs, saved = self._engine.forward(self._tensor_dict(), x, lungs, self.training, True, self._dist,
                                                      self.activation_recompute, self._storage_now(),
                                                      need_x=True, need_param=False)
            for gs, ys, name in ((og, outs, "out_grads"), (dg, dense, "dense_grads")):
                for i, (g, y) in enumerate(zip(gs, ys)):
                    if g is None:
                        continue
                    if not isinstance(g, torch.Tensor) or g.device != y.device or tuple(g.shape) != tuple(y.shape):
                        raise ValueError(f"{name}[{i}]: expected a tensor of shape {tuple(y.shape)} on {y.device}")
                    gs[i] = g.detach().float().contiguous()
            self._engine.backward(saved, dg, og)
        return saved["dx"]

    def _forward_head(self, x, lungs):
        """forward(x, lungs) as it runs under torch.no_grad(), keeping the heads' operands (engine.forward_head)."""
        x = x.detach().contiguous().float()
        if lungs is not None:
            lungs = lungs.detach().contiguous().float()
        with torch.no_grad():
            return self._engine.forward_head(self._tensor_dict(), x, lungs, self.training, self._dist,
                                             self._storage_now())[2]

    def target_activations(self, x: torch.Tensor, lungs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The output of get_target_layer() (us3: conv + BatchNorm + ReLU), the tensor the heads consume, of a forward in
        the module's current mode run as forward() under torch.no_grad() runs it: [B,32,D/2,H/2,W/2] float32 (a permuted
        view of the engine's NDHWC tensor; with bf16 storage the widened copy of what was stored)."""
        self._check_input(x)
        kept = self._forward_head(x, lungs)
        with torch.no_grad(), ops.launch_scope(x.device):
            return ops.cast(kept["xup3"], torch.float32).permute(0, 4, 1, 2, 3)

    def activation_map(self, x: torch.Tensor, lungs: Optional[torch.Tensor] = None, *, out_grads=None, dense_grads=None,
                       score=None, method: str = "gradcam", relu: bool = True,
                       upsample_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Class-activation map of a score s at get_target_layer()'s output A ([B,V,32] per sample), G = ds/dA:
            gradcam   r(sum_c alpha[b,c] A[b,v,c]),  alpha[b,c] = mean_v G[b,v,c]
            hirescam  r(sum_c G[b,v,c] A[b,v,c])
            layercam  r(sum_c max(G[b,v,c], 0) A[b,v,c])            r = ReLU if `relu` else identity
        s is given by cotangents with input_gradient's conventions (out_grads / dense_grads: a pair each, tensor or
        None), or by score=(head, index): outs[head][:, index] of every sample (index 0 or None for the reg networks).
        Runs forward(x, lungs) in the module's current mode as under torch.no_grad() -- no tape, no .grad touched -- and
        forms the map from A in one (hirescam, layercam) or two (gradcam) passes; G is never stored.  Returns
        [B,1,D/2,H/2,W/2] float32, not normalised; with upsample_mask [B,Ds,Hs,Ws] the trilinear (align_corners=True)
        up-sampling to that grid times the mask, [B,1,Ds,Hs,Ws].  Under distributed.attach the result is local to the rank."""
        if method not in ops.CAM_METHODS:
            raise ValueError(f"activation_map: unknown method {method!r} (one of {sorted(ops.CAM_METHODS)})")

        def pair(gs, name):
            gs = [None, None] if gs is None else list(gs)
            if len(gs) != 2:
                raise ValueError(f"{name}: expected two cotangents (or None), got {len(gs)}")
            return gs

        og, dg = pair(out_grads, "out_grads"), pair(dense_grads, "dense_grads")
        reg = self.HEAD == "reg"
        if score is not None:
            if any(g is not None for g in og):
                raise ValueError("activation_map: give score or out_grads, not both")
            head, index = score
            if head not in (0, 1):
                raise ValueError(f"score: head must be 0 or 1, got {head!r}")
            index = 0 if (reg and index is None) else index
            if not isinstance(index, int) or not 0 <= index < self.n_classes[head]:
                raise ValueError(f"score: index {index!r} is outside outs[{head}] ({self.n_classes[head]} columns)")
        elif all(g is None for g in og + dg):
            raise ValueError("activation_map: no score (out_grads, dense_grads and score are all None)")
        if x.dim() == 5:                                # (anything else: _check_input raises below)
            B, grid = x.shape[0], tuple(int(n) // 2 for n in x.shape[-3:])
            out_shapes = [(B,) if reg else (B, n) for n in self.n_classes]
            dense_shapes = [(B, n) + grid for n in self.n_classes]
            for gs, shapes, name in ((og, out_shapes, "out_grads"), (dg, dense_shapes, "dense_grads")):
                for i, (g, shape) in enumerate(zip(gs, shapes)):
                    if g is not None and (not isinstance(g, torch.Tensor) or tuple(g.shape) != shape):
                        raise ValueError(f"{name}[{i}]: expected a tensor of shape {shape}")
            if upsample_mask is not None and (not isinstance(upsample_mask, torch.Tensor) or upsample_mask.dim() != 4
                                              or upsample_mask.shape[0] != B):
                raise ValueError("upsample_mask: expected a tensor [B,Ds,Hs,Ws]")
        self._check_input(x)
        for g in og + dg + [upsample_mask]:
            if g is not None and g.device != x.device:
                raise ValueError(f"activation_map: cotangents and upsample_mask must be on {x.device}")
        if score is not None:
            og[head] = torch.zeros(out_shapes[head], device=x.device)
            og[head][..., index if not reg else slice(None)] = 1.0
        kept = self._forward_head(x, lungs)
        with torch.no_grad():
            og, dg = ([None if g is None else g.detach().float().contiguous() for g in gs] for gs in (og, dg))
            cam = self._engine.activation_map(kept, dg, og, method, bool(relu))
            if upsample_mask is not None:
                with ops.launch_scope(x.device):
                    cam = ops.upproject(cam, upsample_mask.detach().float().contiguous(), tuple(upsample_mask.shape[1:]))[0]
        return cam.unsqueeze(1)


class ResNetSegCls(_ResNetSeg):
    """reference med3d.py:187-285"""
    HEAD = "cls"

    def __init__(self, block, layers, shortcut_type="A", n_classes=[6, 3]):
        super().__init__(block, layers, shortcut_type, n_classes)


class ResNetSegReg(_ResNetSeg):
    """reference med3d.py:288-388"""
    HEAD = "reg"

    def __init__(self, block, layers, shortcut_type="A"):
        super().__init__(block, layers, shortcut_type, (1, 1))


def resnet34segcls(**kwargs):
    return ResNetSegCls(BasicBlock, [3, 4, 6, 3], **kwargs)


def resnet50segcls(**kwargs):
    return ResNetSegCls(Bottleneck, [3, 4, 6, 3], **kwargs)


def resnet18segcls(**kwargs):
    return ResNetSegCls(BasicBlock, [2, 2, 2, 2], **kwargs)


def resnet34segreg(**kwargs):
    return ResNetSegReg(BasicBlock, [3, 4, 6, 3], **kwargs)


def resnet50segreg(**kwargs):
    return ResNetSegReg(Bottleneck, [3, 4, 6, 3], **kwargs)


def resnet18segreg(**kwargs):
    return ResNetSegReg(BasicBlock, [2, 2, 2, 2], **kwargs)
