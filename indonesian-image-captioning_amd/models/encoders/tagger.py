"""EncoderTagger on MI355X: drop-in for the reference's models/encoders/tagger.py.

(B,3,H,W) images -> ResNet-152 trunk INCLUDING the global average pool -> (B,2048) -> Dropout(0.15) ->
Linear(2048, semantic_size) -> Sigmoid = tag probabilities (B, semantic_size), which the train step feeds
to the decoder as `semantic_input` (trains/attention_scn.py:214).  Same module tree / state_dict keys as
the reference (`resnet.<idx>...`, `linear.{weight,bias}`); the trunk is scnattn.resnet (the hand-written
convolution kernels with the BatchNorm fused into them, in training and in eval mode), the Linear runs on the MFMA sgemm."""
import torch
from torch import nn

from scnattn import functional as SF
from scnattn.resnet import resnet152_trunk, configure_miopen, manage_bn_counters
from scnattn.stem import run_trunk, usable as stem_usable

configure_miopen()


class EncoderTagger(nn.Module):
    def __init__(self, semantic_size=1000, dropout=0.15, channels_last=False):
        super().__init__()
        self.semantic_size = semantic_size
        self.resnet = resnet152_trunk(keep_avgpool=True)   # children()[:-1] of torchvision's resnet152
        self.dropout = nn.Dropout(dropout)
        self.linear = nn.Linear(2048, semantic_size)
        self.sigmoid = nn.Sigmoid()
        self.channels_last = channels_last
        self.fine_tune()

    def forward(self, images):
        if self.channels_last and images.is_cuda and not stem_usable(self.resnet, images):      # the fused stem reads any strides
            images = images.contiguous(memory_format=torch.channels_last)
        if images.is_cuda and self.training:
            flat = getattr(self, "_bn_counters", None)
            if flat is None or flat.device != images.device:
                self._bn_counters = flat = manage_bn_counters(self.resnet)
            if flat is not None:
                flat.add_(1)
        out = run_trunk(self.resnet, images)      # stem on csrc/stem.hip, Bottlenecks on scnattn/conv.py (conv16.py in bf16)
        out = out.float()
        out = out.reshape(out.size(0), -1)
        out = self.dropout(out)
        out = SF.linear(out, self.linear.weight, self.linear.bias)
        return self.sigmoid(out)

    def tag_loss(self, images, targets, loss=None):
        """One call for the train step and validation of trains/tagger.py:161-163,176: (probs, loss, agree) with
        probs = forward(images), loss = nn.BCELoss()(probs, targets) and agree = binary_accuracy's count of
        (probs >= 0.5) == (targets >= 0.5), the last two as 0-d device tensors.  The trunk is the one `forward` runs; pool,
        dropout mask, sigmoid, loss and count run on csrc/taghead.hip (scnattn.functional.tag_head_loss).  `loss`: a
        scnattn.functional.TagLoss in the place of nn.BCELoss (weights, focal, asymmetric); probs and agree stay what they are."""
        SF.require_cuda(images, targets)
        if self.channels_last and not stem_usable(self.resnet, images):
            images = images.contiguous(memory_format=torch.channels_last)
        if self.training:
            flat = getattr(self, "_bn_counters", None)
            if flat is None or flat.device != images.device:
                self._bn_counters = flat = manage_bn_counters(self.resnet)
            if flat is not None:
                flat.add_(1)
        # the trunk's parameters, listed once per trunk object: walking ~500 modules costs 0.3 ms of host time per step
        cached = self.__dict__.get("_trunk_info")
        if cached is None or cached[0] is not self.resnet:
            pooled = isinstance(list(self.resnet.children())[-1], nn.AdaptiveAvgPool2d)     # the fused head pools the map itself
            cached = self.__dict__["_trunk_info"] = (self.resnet, pooled, tuple(self.resnet.parameters()))
        _, pooled, params = cached
        # a frozen trunk keeps nothing for a backward pass that never comes
        trains = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        with torch.set_grad_enabled(trains):
            x4 = run_trunk(self.resnet, images, drop_last=1 if pooled else 0)
        ks = None
        if self.training:       # the module's own draw, pre-scaled by 1 / (1 - p); honours a replaced dropout module
            ks = self.dropout(torch.ones(x4.shape[0], x4.shape[1], device=x4.device))
        # a bf16 map (bf16 autocast): forward()'s pool hands its mean on in bf16; the step trains the function forward() evaluates
        return SF.tag_head_loss(x4, ks, self.linear.weight, self.linear.bias, targets, pooled_bf16=x4.dtype == torch.bfloat16,
                                loss=loss)

    def fine_tune(self, fine_tune=True):
        for p in self.resnet.parameters():
            p.requires_grad = False
        for child in list(self.resnet.children())[5:]:
            for p in child.parameters():
                p.requires_grad = fine_tune

    def to(self, *args, **kwargs):
        m = super().to(*args, **kwargs)
        if self.channels_last and any(p.is_cuda for p in m.parameters()):
            m.resnet.to(memory_format=torch.channels_last)
        return m
