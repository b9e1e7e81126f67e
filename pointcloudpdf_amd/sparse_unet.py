"""SpUNet-v1m1 -- pointcept/models/sparse_unet/spconv_unet_v1m1_base.py (``SpUNetBase``): the sparse-convolution U-Net of the
``semseg-spunet-*`` / ``cls-spunet`` / ``semseg-cac-v1m1-*-spunet-*`` recipes, over this package's own sparse convolutions
(sparse_conv.py, csrc/sparse_conv.hip) instead of spconv.  Same constructor, submodule tree and ``state_dict`` keys
(``conv_input.0.weight``, ``down.{s}.0``, ``enc.{s}.block{i}.conv1``, ``...proj.0``, ``up.{s}.0``, ``dec.{s}.block{i}``, ``final``),
``BatchNorm1d(eps=1e-3, momentum=0.01)`` through dense.bn_act, ``trunc_normal_(std=0.02)`` on the SubM weights.

The geometry of all levels depends on the coordinates alone: ``SpUNetBase.make_geometry(grid_coord, offset)`` builds it ahead of the
forward (one submission, one host read) and the forward takes it from ``data_dict["spunet_geometry"]``; without the key the forward
builds the same object itself (bit-identical results)."""
from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn

from . import dense
from . import sparse_conv as spconv
from .registry import MODELS


def _trunc_normal_(w, std=0.02):
    return nn.init.trunc_normal_(w, std=std, a=-2.0, b=2.0)


class BasicBlock(spconv.SparseModule):
    """conv1 - bn1 - relu - conv2 - bn2, + proj(x), relu (both convolutions 3x3x3 SubM on the block's level)."""

    expansion = 1

    def __init__(self, in_channels, embed_channels, stride=1, norm_fn=None, indice_key=None, bias=False):
        super().__init__()
        assert norm_fn is not None
        if in_channels == embed_channels:
            self.proj = spconv.SparseSequential(nn.Identity())
        else:
            self.proj = spconv.SparseSequential(spconv.SubMConv3d(in_channels, embed_channels, kernel_size=1, bias=False),
                                                norm_fn(embed_channels))
        self.conv1 = spconv.SubMConv3d(in_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias, indice_key=indice_key)
        self.bn1 = norm_fn(embed_channels)
        self.relu = nn.ReLU()
        self.conv2 = spconv.SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias,
                                       indice_key=indice_key)
        self.bn2 = norm_fn(embed_channels)
        self.stride = stride

    def forward(self, x):
        out = self.conv1(x)
        out = out.replace_feature(dense.bn_act(self.bn1, out.features.contiguous(), relu=True))
        out = self.conv2(out)
        res = self.proj(x).features
        return out.replace_feature(dense.bn_act(self.bn2, out.features.contiguous(), residual=res.contiguous(), relu=True))


@MODELS.register_module("SpUNet-v1m1")
class SpUNetBase(nn.Module):
    def __init__(self, in_channels, num_classes, base_channels=32, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                 layers=(2, 3, 4, 6, 2, 2, 2, 2), cls_mode=False):
        super().__init__()
        assert len(layers) % 2 == 0
        assert len(layers) == len(channels)
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.base_channels = base_channels
        self.channels = channels
        self.layers = layers
        self.num_stages = len(layers) // 2
        self.cls_mode = cls_mode

        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        self.conv_input = spconv.SparseSequential(
            spconv.SubMConv3d(in_channels, base_channels, kernel_size=5, padding=1, bias=False, indice_key="stem"),
            norm_fn(base_channels), nn.ReLU())

        enc_channels = base_channels
        dec_channels = channels[-1]
        self.down = nn.ModuleList()
        self.up = nn.ModuleList()
        self.enc = nn.ModuleList()
        self.dec = nn.ModuleList() if not self.cls_mode else None
        for s in range(self.num_stages):
            self.down.append(spconv.SparseSequential(
                spconv.SparseConv3d(enc_channels, channels[s], kernel_size=2, stride=2, bias=False, indice_key=f"spconv{s + 1}"),
                norm_fn(channels[s]), nn.ReLU()))
            self.enc.append(spconv.SparseSequential(OrderedDict(
                (f"block{i}", BasicBlock(channels[s], channels[s], norm_fn=norm_fn, indice_key=f"subm{s + 1}")) for i in range(layers[s]))))
            if not self.cls_mode:
                self.up.append(spconv.SparseSequential(
                    spconv.SparseInverseConv3d(channels[len(channels) - s - 2], dec_channels, kernel_size=2, bias=False,
                                               indice_key=f"spconv{s + 1}"),
                    norm_fn(dec_channels), nn.ReLU()))
                self.dec.append(spconv.SparseSequential(OrderedDict(
                    (f"block{i}", BasicBlock(dec_channels + enc_channels if i == 0 else dec_channels, dec_channels, norm_fn=norm_fn,
                                             indice_key=f"subm{s}")) for i in range(layers[len(channels) - s - 1]))))
            enc_channels = channels[s]
            dec_channels = channels[len(channels) - s - 2]

        final_in_channels = channels[-1] if not self.cls_mode else channels[self.num_stages - 1]
        self.final = (spconv.SubMConv3d(final_in_channels, num_classes, kernel_size=1, padding=1, bias=True) if num_classes > 0
                      else spconv.Identity())
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear) or isinstance(m, spconv.SubMConv3d):
            _trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @staticmethod
    def _indices(grid_coord, offset):
        n = grid_coord.shape[0]
        batch = torch.searchsorted(offset.long(), torch.arange(n, device=offset.device), right=True)   # offset2batch without a host read
        return torch.cat([batch.unsqueeze(-1).int(), grid_coord.int()], dim=1).contiguous()

    def make_geometry(self, grid_coord, offset):
        """The tables of every level (coordinate-only): hand the result in as ``data_dict["spunet_geometry"]``."""
        levels = self.num_stages + 1
        sizes = [(5, 3)] + [(3,)] * (levels - 1)
        # No spatial_shape: the reference passes max(grid_coord) + 96, which halves to a margin of 6 cells at level 4, so spconv's
        # truncation of output sites outside shape // 2 never fires; unbounded is the same function.
        return spconv.SpGeometry.build(self._indices(grid_coord, offset), levels, sizes, None)

    @dense.fp32_path
    def forward(self, input_dict):
        grid_coord = input_dict["grid_coord"]
        feat = input_dict["feat"]
        offset = input_dict["offset"]
        geometry = input_dict.get("spunet_geometry")
        if geometry is None:
            geometry = self.make_geometry(grid_coord, offset)
        indices = geometry.indices0
        if indices.shape[0] != feat.shape[0]:
            raise ValueError(f"SpUNet-v1m1: the geometry holds {indices.shape[0]} sites, feat {feat.shape[0]} rows")
        x = spconv.SparseConvTensor(features=feat, indices=indices, spatial_shape=None, batch_size=offset.shape[0], geometry=geometry)
        x = self.conv_input(x)
        skips = [x]
        for s in range(self.num_stages):
            x = self.down[s](x)
            x = self.enc[s](x)
            skips.append(x)
        x = skips.pop(-1)
        if not self.cls_mode:
            for s in reversed(range(self.num_stages)):
                x = self.up[s](x)
                skip = skips.pop(-1)
                x = x.replace_feature(torch.cat((x.features, skip.features), dim=1))
                x = self.dec[s](x)
        x = self.final(x)
        if self.cls_mode:
            # per-scene mean (torch_geometric's scatter(reduce="mean") over the batch index)
            b = x.indices[:, 0].long()
            sums = x.features.new_zeros((offset.shape[0], x.features.shape[1])).index_add(0, b, x.features)
            cnt = torch.bincount(b, minlength=offset.shape[0]).clamp(min=1).to(sums.dtype)
            return sums / cnt.unsqueeze(1)
        return x.features
