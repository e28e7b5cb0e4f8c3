"""The C ABI's buffer contract (include/btcdet_hip.h, "Rules common to every entry point"): helpers and the case table.

Every output of a contract case is a `Guarded` buffer: one device allocation laid out as [front guard | payload | back guard], the
payload filled with a poison no valid result equals, the guards with a second pattern.  A slot the kernel leaves unwritten still
holds the poison; a write past either end of the payload lands in a guard (memory this allocation owns) and shows up in
`guards_intact()`.  Every workspace is a `Workspace`: the documented zero head zeroed, the rest garbage (0xA5 or 0xFF -- 0xFF reads
as -1, a valid map value), so a kernel that relies on workspace state it did not write itself is caught.

CASES names every compute entry point the header declares, grouped by the case of tests/test_hip_abi_contract.py that calls it;
tests/test_abi_contract_cpu.py checks it against the header.  This module imports nothing that needs a GPU at import time.
"""
GUARD = 4096                      # bytes per guard band: keeps the payload 256-byte aligned
GUARD_BYTE = 0x3C                 # the guards' pattern (differs from every poison and garbage byte)

# poison of the payload, per element type: a pattern no valid result can equal
POISON = {
    "float32": 0x7FC5A5A5,        # a quiet NaN with a payload
    "bfloat16": 0x7FC5,           # the bf16 quiet NaN of the same payload
    "int32": 0x5A5A5A5A,          # not -1: cannot pass as an absent neighbour
    "int64": 0x5A5A5A5A5A5A5A5A,
    "uint8": 0xA5,
    "int8": 0xA5,
}
GARBAGE = (0xA5, 0xFF)

# case -> the entry points it calls; every compute entry point of include/btcdet_hip.h is named here exactly once or more
CASES = {
    "voxelize": ("btc_voxelize",),
    "range_mask_gather": ("btc_range_mask_compact", "btc_gather_rows"),
    "cart_to_occ_coords": ("btc_cart_to_occ_coords",),
    "voxel_shift_col": ("btc_voxel_shift_col",),
    "rulebook_subm": ("btc_rulebook_subm",),
    "rulebook_conv": ("btc_rulebook_conv_count", "btc_rulebook_conv_fill"),
    "chain": ("btc_chain_levels", "btc_chain_maps"),
    "pairs_from_nbr": ("btc_pairs_from_nbr",),
    "row_orders": ("btc_row_orders", "btc_row_orders_keyed"),
    "conv_fwd_dgrad": ("btc_conv_fwd", "btc_conv_dgrad", "btc_conv_fwd_bf16", "btc_conv_dgrad_bf16"),
    "conv_bf16w": ("btc_weights_to_bf16", "btc_weights_to_bf16_multi", "btc_conv_fwd_bf16w", "btc_conv_dgrad_bf16w"),
    "conv_apply": ("btc_conv_apply_ordered", "btc_conv_apply_src", "btc_weights_split3", "btc_weights_split3_multi"),
    "conv_bn_relu": ("btc_conv_bn_relu_fwd", "btc_conv_bn_relu_fwd_src"),
    "conv_wgrad": ("btc_conv_wgrad", "btc_conv_wgrad_bf16", "btc_conv_wgrad_ordered", "btc_conv_wgrad_slabs",
                   "btc_wgrad_reduce_multi"),
    "maxpool": ("btc_maxpool_fwd", "btc_maxpool_bwd"),
    "dense": ("btc_dense_fwd", "btc_dense_bwd", "btc_dense_split_fwd", "btc_dense_split_bwd"),
    "cat_pad": ("btc_cat_pad_fwd", "btc_cat_pad_bwd"),
    "bn_relu": ("btc_bn_relu_fwd", "btc_bn_relu_bwd", "btc_bn_relu_fwd_bf16", "btc_bn_relu_bwd_bf16"),
    "col_sum": ("btc_col_sum", "btc_col_sum_bf16"),
    "sumsq2": ("btc_sumsq2_fwd", "btc_sumsq2_bwd"),
    "occ_targets": ("btc_occ_targets", "btc_occ_backproject_lut"),
    "occ_prob": ("btc_occ_prob",),
    "occ_loss": ("btc_occ_loss_fwd", "btc_occ_loss_bwd", "btc_occ_loss_fwd_total", "btc_occ_loss_bwd_total"),
    "vfe": ("btc_mean_vfe", "btc_occ_vfe"),
    "pass_occ_vox": ("btc_pass_occ_vox_count", "btc_pass_occ_vox_fill", "btc_pass_occ_vox_fill_i32"),
    "revoxelize": ("btc_revoxelize_count", "btc_revoxelize_fill"),
    "boxes_nms": ("btc_boxes_pairwise_bev", "btc_nms", "btc_nms_topk"),
    "ball_group": ("btc_ball_query", "btc_group_points", "btc_group_points_grad"),
    "fps": ("btc_furthest_point_sampling",),
    "three_nn_interp": ("btc_three_nn", "btc_three_interpolate", "btc_three_interpolate_grad"),
    "trilinear": ("btc_trilinear_corners", "btc_trilinear_gather", "btc_trilinear_scatter"),
    "adam": ("btc_adam_group_step", "btc_grads_pack"),
}


# ---------------------------------------------------------------------------------------------------------------------- device side
def _torch():
    import torch
    return torch


def _dtype(dt):
    torch = _torch()
    return {"float32": torch.float32, "bfloat16": torch.bfloat16, "int32": torch.int32, "int64": torch.int64,
            "uint8": torch.uint8, "int8": torch.int8}[dt] if isinstance(dt, str) else dt


def _dname(dt):
    return str(dt).replace("torch.", "")


def fill_bytes(t, pattern, elem_bytes):
    """fill tensor t (any dtype) with the little-endian integer `pattern` of elem_bytes bytes"""
    torch = _torch()
    raw = t.view(torch.uint8).view(-1)
    if raw.numel() == 0:
        return
    b = torch.tensor(list(int(pattern).to_bytes(elem_bytes, "little")), dtype=torch.uint8, device=t.device)
    raw.view(-1, elem_bytes).copy_(b.expand(raw.numel() // elem_bytes, elem_bytes))


def poison_like(t):
    """fill t with the poison of its dtype (in place); returns t"""
    name = _dname(t.dtype)
    fill_bytes(t, POISON[name], t.element_size())
    return t


class Guarded(object):
    """Guarded(shape, dtype) or Guarded(nbytes): [GUARD | payload | GUARD] in one device allocation, payload poisoned"""

    def __init__(self, shape, dtype="uint8", device="cuda", fill=None):
        torch = _torch()
        if isinstance(shape, int):
            shape = (shape,)
        self.dtype = _dtype(dtype)
        self.shape = tuple(int(s) for s in shape)
        esz = torch.empty((), dtype=self.dtype).element_size()
        n = 1
        for s in self.shape:
            n *= s
        self.nbytes = n * esz
        pay = (self.nbytes + 255) & ~255
        self.raw = torch.empty((2 * GUARD + pay,), dtype=torch.uint8, device=device)
        self.raw.fill_(GUARD_BYTE)
        self.tensor = self.raw[GUARD:GUARD + self.nbytes].view(self.dtype).view(self.shape)
        if fill is None:
            poison_like(self.tensor)
        else:
            self.tensor.fill_(fill)
        self.pad = pay - self.nbytes           # bytes between the payload's end and the back guard: must stay GUARD_BYTE too

    @property
    def ptr(self):
        return self.tensor.data_ptr()

    def guards_intact(self):
        torch = _torch()
        front = self.raw[:GUARD]
        back = self.raw[GUARD + self.nbytes:]
        return bool(torch.all(front == GUARD_BYTE)) and bool(torch.all(back == GUARD_BYTE))

    def poison_mask(self):
        """bool tensor of self.shape: element still holds the poison (bitwise)"""
        torch = _torch()
        ref = poison_like(torch.empty((1,), dtype=self.dtype, device=self.tensor.device))
        ib = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.tensor.element_size()]
        return self.tensor.view(ib) == ref.view(ib)[0]


class Workspace(Guarded):
    """Workspace(nbytes, zero_head=N, garbage=0xA5|0xFF): guarded bytes, the first zero_head zero, the rest garbage"""

    def __init__(self, nbytes, zero_head=0, garbage=0xA5, device="cuda"):
        super(Workspace, self).__init__((max(int(nbytes), 1),), "uint8", device, fill=garbage)
        self.ws_bytes = int(nbytes)
        self.zero_head = int(zero_head)
        if zero_head:
            self.tensor[:zero_head].zero_()

    def head_zero(self):
        torch = _torch()
        return bool(torch.all(self.tensor[:self.zero_head] == 0))


def call(name, *args):
    """one entry point through ctypes on a non-default stream; syncs that stream only; asserts rc == 0"""
    torch = _torch()
    from btcdet_amd import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    torch.cuda.current_stream().synchronize()      # inputs made on the current stream are ready
    s = torch.cuda.Stream()
    rc = fn(*args, s.cuda_stream)
    s.synchronize()
    assert rc == 0, "%s returned %d: %s" % (name, rc, L.btc_last_error().decode("utf-8", "replace"))
    return rc
