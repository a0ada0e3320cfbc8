"""ModelInputs: one forward's inputs in the form every model entry of the C-ABI takes them."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .context import ptr
from .graph import EdgeList


@dataclass
class ModelInputs:
    """fp32, contiguous, on the engine's device (DynamicsPredictor._inputs builds and checks them)."""
    state: torch.Tensor     # (B, n_his, N, 3)
    attrs: torch.Tensor     # (B, N, 2)
    action: torch.Tensor    # (B, N, 3)
    phys: torch.Tensor      # (B, N): the physics parameter per particle, 0 on the tool rows
    group: torch.Tensor     # (B, N, n_inst): p_instance, 0 on the tool rows
    edges: EdgeList
    n_p: int

    B = property(lambda self: self.attrs.shape[0])
    N = property(lambda self: self.attrs.shape[1])
    n_inst = property(lambda self: self.group.shape[2])

    def c_args(self):
        """The 14 arguments behind (ctx, stream) of ag_forward, ag_backward, ag_backward_inputs and ag_train_step*."""
        return (ptr(self.state), ptr(self.attrs), ptr(self.action), ptr(self.phys), ptr(self.group), self.n_inst,
                ptr(self.edges.recv), ptr(self.edges.send), ptr(self.edges.row_ptr), ptr(self.edges.n_edges),
                self.edges.edge_cap, self.B, self.N, self.n_p)
