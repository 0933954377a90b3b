"""Visualise latent space by blending many output samples per pixel (reference explore/continuous_interp.py).

A ``num_points`` x ``num_points`` slerp grid of latents (or, under ``--tile``, the 3 x 3 arrangement of nine corner latents that
wraps around) is rendered one grid ROW per generator call, in ascending order and only the rows the mosaic reads -- a train-mode
generator's BatchNorm statistics depend on exactly that batching, so it is kept.  The reference then copies ``output_size`` squared
single pixels from the device to a host image; here the mosaic is ONE gather (``tg_mosaic_gather``), whose integer index
``(y * rows) // S`` equals the reference's ``int(y * rows / S)`` everywhere in range.
"""
import torch

from .. import functional as TF
from ..trainers.components.image_sampler import slerp_grid
from .base import GOutputApp, set_device_from_args


class ContinuousInterp(GOutputApp):
    """Visualize latent space by blending many output samples per pixel"""
    app_name = 'Continuous Interplotion'

    @torch.no_grad()
    def run(self):
        set_device_from_args(self.args)
        self.load_generator()
        self.make_output_dir()
        if self.args.tile:
            grid = self.unmirrored_tiled_grid(self.args.num_points, self.args.num_points)
        else:
            grid = self.sample_latent_grid(self.args.num_points, self.args.num_points)
        rows, cols = grid.shape[:2]
        size = self.args.output_size
        grid_imgs = None
        for grid_y in sorted({TF.mosaic_index(y, rows, size) for y in range(size)}):
            row_imgs = self.g(grid[grid_y])
            if grid_imgs is None:          # rows the mosaic never reads (output_size < rows) are not rendered and stay zero
                grid_imgs = row_imgs.new_zeros((rows, cols) + tuple(row_imgs.shape[1:]))
            grid_imgs[grid_y] = row_imgs
        output_img = TF.mosaic_gather(grid_imgs.view((rows * cols,) + tuple(grid_imgs.shape[2:])), rows, cols, size)
        self.save_image(output_img, f'{self.args.output_prefix}_combined.png')
        return output_img

    def _corners(self, n):
        return [z.cpu().numpy() for z in self.sample_z(n)]

    def sample_latent_grid(self, nrows, ncols):
        top_left, top_right, bottom_left, bottom_right = self._corners(4)
        grid = slerp_grid(top_left, top_right, bottom_left, bottom_right, nrows, ncols)
        return grid.to(self.args.device, torch.float32).view(nrows, ncols, -1)

    def unmirrored_tiled_grid(self, nrows, ncols):
        """A 3 x 3 table of nine latents, wrapped around: tile (r, c) is the slerp grid between table entries (r, c), (r, c + 1),
        (r + 1, c) and (r + 1, c + 1), indexes modulo 3, a third of the points along each side, without its last row and column
        (the next tile starts there).  The mosaic's right and bottom edges therefore continue into its left and top ones."""
        tile_rows, tile_cols = nrows // 3 - 1, ncols // 3 - 1
        table = self._corners(9)

        def corner(r, c):
            return table[(r % 3) * 3 + c % 3]

        grid = torch.zeros(3 * tile_rows, 3 * tile_cols, table[0].shape[0])
        for r in range(3):
            for c in range(3):
                tile = slerp_grid(corner(r, c), corner(r, c + 1), corner(r + 1, c), corner(r + 1, c + 1), tile_rows + 1, tile_cols + 1)
                tile = tile.view(tile_rows + 1, tile_cols + 1, -1)[:tile_rows, :tile_cols]
                grid[r * tile_rows:(r + 1) * tile_rows, c * tile_cols:(c + 1) * tile_cols] = tile
        return grid.to(self.args.device)

    @classmethod
    def add_args_to_parser(cls, p):
        super().add_args_to_parser(p)
        p.add_argument('--output-size', default=256, type=int)
        p.add_argument('--num-points', type=int, default=6, help='Number of points to visit')
        p.add_argument('--tile', action='store_true')


if __name__ == '__main__':
    ContinuousInterp.run_from_cli()
