"""TEST INFRASTRUCTURE ONLY -- a plain torch restatement of the reference lines moco_flow_amd.batch replaces.  The reference's
dataset module cannot be imported here (it needs cv2 and trimesh, which this project does not have), so this file RESTATES
those lines; every function names the lines it restates and keeps their operations in their order:

    to_tensor        torchvision.transforms.ToTensor on an 8-bit HWC image: permute to CHW, .float().div(255)
    composite        datasets/moco_flow_dataset.py:169-176 -- img[:3] * img[-1:] + bkgd_img * (1 - img[-1:]), then
                     .view(3, -1).permute(1, 0) for the (H W, 3) rows of the image and of the background
    select           trainer/trainer_moco_flow.py:414-416 -- val_inds = torch.nonzero(rays_msk).squeeze(1),
                     sel_inds = val_inds[perm[:N_rand]], and the three gathers
    chain_column     trainer/trainer_moco_flow.py:308-312 -- torch.cat([rays, chain_idx * torch.ones_like(rays[:, :1])], 1)

Everything runs on the device of its inputs, in fp32, one torch op per reference op (torch does not fuse a multiply into an
add), so the comparison with the kernel is torch.equal."""
import torch


def to_tensor(u8_hwc):
    """(H, W, C) uint8 -> (C, H, W) fp32 in [0, 1]."""
    return u8_hwc.permute(2, 0, 1).contiguous().float().div(255)


def background_image(background, H, W):
    """bkgd_img (3, H, W): one (3,) colour repeated over the frame (moco_flow_dataset.py:173 builds it with
    .repeat(1, *size)), or (H W, 3) rows put back into planes."""
    if background.dim() == 1:
        return background.view(3, 1, 1).repeat(1, H, W)
    return background.view(H, W, 3).permute(2, 0, 1)


def rows(chw):
    """moco_flow_dataset.py:175-176: .view(3, -1).permute(1, 0)."""
    return chw.reshape(3, -1).permute(1, 0)


def composite(u8_hwc, background, H, W):
    """moco_flow_dataset.py:169-176 -> (rgbs (H W, 3), background (H W, 3) or None)."""
    img = to_tensor(u8_hwc)
    bkgd_img = None if background is None else background_image(background, H, W)
    if img.shape[0] == 4:
        img = img[:3, ...] * img[-1:, ...] + bkgd_img * (1 - img[-1:, ...])
    return rows(img), None if bkgd_img is None else rows(bkgd_img)


def val_inds(rays_msk):
    """trainer_moco_flow.py:414."""
    return torch.nonzero(rays_msk).squeeze(1)


def select(rays, rays_msk, rgbs, background, perm, N_rand):
    """trainer_moco_flow.py:414-416 with the permutation passed in -> (rays, rgbs, background, sel_inds)."""
    inds = val_inds(rays_msk)
    sel_inds = inds[perm[:N_rand]]
    pick = lambda t: None if t is None else t[sel_inds]
    return rays[sel_inds], pick(rgbs), pick(background), sel_inds


def chain_column(rays, chain_idx):
    """trainer_moco_flow.py:310-312."""
    return torch.cat([rays, chain_idx * torch.ones_like(rays[:, :1])], dim=1)
