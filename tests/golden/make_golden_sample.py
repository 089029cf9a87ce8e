"""Golden vectors for the plain N_rand sampling path (invr.trainset mode 'plain' / include/invr_sample.h), produced by the REFERENCE's
own sample_ray_h36m (lib/utils/if_nerf/if_nerf_data_utils.py:228-297) under recorded NumPy seeds, on the synthetic scenes of
tests/patch_reference.py with an orig_msk added (tests/sample_reference.py: synthetic_orig_msk, with_face).
Run on the CPU machine only:  python tests/golden/make_golden_sample.py
trimesh is stubbed (unused here).  cv2 is stubbed with a fillPoly of OUR OWN — the closed even-odd fill of the given integer polygon
(a pixel is set iff it lies on an edge or the crossing-number rule puts it inside), in exact integer arithmetic — so this golden pins
everything AFTER the bound mask (classes, draws, rounds, rays, near / far, pixels), not cv2's rasteriser; the mask the reference built
with that fill is stored per scene and asserted equal to the hull mask of the restatement.
np.random.randint is wrapped while the reference runs to record its calls: the round structure stored per case is the restatement's,
after its implied call sequence has been held against the recorded one.
Stored: per scene the camera, the box, the image seed, the face switch and the bound mask; per case the seed, N_rand, the two ratios,
the rounds and the reference's coord / ray_d / near / far with occupancy = orig_msk[coord] (tpose_dataset.py:450)."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden as mg   # noqa: E402

# the patch fixtures' scenes ('b': the box is cut by the frame's edge); 'f' is 'a' with a face class
SCENES = {'a': dict(H=160, W=128, cam_dist=2.2, img_seed=11, face=0),
          'b': dict(H=96, W=80, cam_dist=1.6, img_seed=12, face=0),
          'f': dict(H=160, W=128, cam_dist=2.2, img_seed=14, face=1)}
# (scene, N_rand, body ratio, face ratio, what the case is there for); the seed of each is searched below, smallest first
# (in 'a' and 'f' 173 pixels of the hull have a ray that misses the box — rounding the corners moves the outline — so a draw of 1024
# needs a second round by itself; in 'b' none has, every draw there is a single round)
WANTED = [('a', 100, 0.5, 0.0, 'one_round'), ('a', 1024, 0.5, 0.0, 'two_rounds'), ('f', 1024, 0.5, 0.25, 'face'), ('a', 100, 0.5, 0.25, 'empty_face'), ('b', 1, 0.5, 0.0, 'any'), ('f', 100, 0.3, 0.3, 'face'),
          ('b', 1024, 0.5, 0.0, 'one_round')]


def fill_poly(mask, polys, color):
    """Closed even-odd fill of integer polygons into mask (H,W), in place."""
    H, W = mask.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    for poly in polys:
        p = np.asarray(poly, np.int64).reshape(-1, 2)
        inside, on = np.zeros((H, W), bool), np.zeros((H, W), bool)
        for (ax, ay), (bx, by) in zip(p, np.roll(p, -1, axis=0)):
            cr = (bx - ax) * (yy - ay) - (by - ay) * (xx - ax)
            on |= (cr == 0) & (xx >= min(ax, bx)) & (xx <= max(ax, bx)) & (yy >= min(ay, by)) & (yy <= max(ay, by))
            inside ^= ((ay <= yy) & (by > yy) & (cr > 0)) | ((by <= yy) & (ay > yy) & (cr < 0))
        mask[inside | on] = color
    return mask


def main():
    sys.modules['trimesh'] = types.ModuleType('trimesh')
    cv2 = types.ModuleType('cv2')
    cv2.fillPoly = fill_poly
    sys.modules['cv2'] = cv2
    rcfg = mg.import_reference(16)
    from lib.utils.if_nerf import if_nerf_data_utils as du
    import invr  # noqa: F401
    from invr import scene
    from tests import patch_reference as P
    from tests import sample_reference as S

    real_randint = np.random.randint

    def item(sc, n_rand, body_ratio, face_ratio, seed):
        """One call of the reference's sample_ray_h36m on the synthetic frame `sc` -> its outputs and its randint calls (high, size)."""
        rcfg.body_sample_ratio, rcfg.face_sample_ratio = body_ratio, face_ratio
        calls = []

        def randint(low, high=None, size=None, *a, **k):
            calls.append((int(high), int(size)))
            return real_randint(low, high, size, *a, **k)
        np.random.seed(seed)
        np.random.randint = randint
        try:
            rgb, ray_o, ray_d, near, far, coord, mask_at_box = du.sample_ray_h36m(sc['img'].copy(), sc['msk'].copy(), sc['K'].copy(), sc['R'].copy(),
                                                                                  sc['T'].copy(), sc['wbounds'].copy(), n_rand, 'train')
        finally:
            np.random.randint = real_randint
        return dict(rgb=rgb, ray_o=ray_o, ray_d=ray_d, near=near, far=far, coord=coord, mask_at_box=mask_at_box, calls=calls,
                    occupancy=sc['orig_msk'][coord[:, 0], coord[:, 1]])

    out = {}
    for tag, sc in SCENES.items():
        b, ex = scene.make_scene(sc['H'], sc['W'], seed=0, cam_dist=sc['cam_dist'])
        sc.update(K=ex['K'], R=ex['Rc'], T=ex['Tc'], wbounds=b['wbounds'][0])
        msk, _ = P.synthetic_masks(sc['H'], sc['W'])
        sc['msk'] = S.with_face(msk, sc['H'], sc['W']) if sc['face'] else msk
        sc['orig_msk'] = S.synthetic_orig_msk(sc['msk'])
        sc['img'] = P.synthetic_image(sc['H'], sc['W'], sc['img_seed'], sc['msk'])
        pose = np.concatenate([sc['R'], sc['T']], axis=1)
        sc['bound'] = du.get_bound_2d_mask(sc['wbounds'], sc['K'], pose, sc['H'], sc['W'])
        mine = S.bound_mask(sc['wbounds'], sc['K'], sc['R'], sc['T'], sc['H'], sc['W'])
        assert np.array_equal(mine, sc['bound']), (tag, 'the hull differs from the six filled faces on', np.argwhere(mine != sc['bound']))
        coords = S.classes(sc['msk'], sc['bound'])
        rays_o, rays_d = S.frame_rays(sc['H'], sc['W'], sc['K'], sc['R'], sc['T'])
        sc['inside'] = S.near_far(sc['wbounds'], rays_o, rays_d.reshape(-1, 3))[2].reshape(sc['H'], sc['W'])
        sc['coords'] = coords
        print('scene', tag, 'classes', [len(c) for c in coords], 'members outside the box', [int((~sc['inside'][c[:, 0], c[:, 1]]).sum()) for c in coords],
              'bound cut by the frame edge', bool(sc['bound'][0].any() or sc['bound'][-1].any() or sc['bound'][:, 0].any() or sc['bound'][:, -1].any()))
        assert (len(coords[1]) > 0) == bool(sc['face'])
        for k in ('K', 'R', 'T', 'wbounds'):
            out['%s_%s' % (tag, k)] = sc[k]
        out[tag + '_meta'] = np.array([sc['H'], sc['W'], sc['img_seed'], sc['face']])
        out[tag + '_bound'] = np.packbits(sc['bound'])

    used, names, max_ulp = set(), [], 0
    for n, (tag, n_rand, body_ratio, face_ratio, want) in enumerate(WANTED):
        sc = SCENES[tag]
        for seed in range(4000):
            if (tag, seed) in used:
                continue
            mine = S.plain_batch(sc['img'], sc['msk'], sc['orig_msk'], sc['K'], sc['R'], sc['T'], sc['wbounds'], n_rand, body_ratio, face_ratio,
                                 np.random.RandomState(seed), bound=sc['bound'])
            rounds = mine['rounds']
            ok = {'one_round': len(rounds) == 1, 'two_rounds': len(rounds) >= 2, 'any': True,
                  'face': rounds[0][1] > 0 and (mine['sel'][:, 0] == 1).any(),
                  'empty_face': rounds[0][1] == -1 and len(rounds) >= 2}[want]
            if ok:
                break
        else:
            raise RuntimeError('no seed found for %r' % ((tag, n_rand, body_ratio, face_ratio, want),))
        used.add((tag, seed))
        r = item(sc, n_rand, body_ratio, face_ratio, seed)
        name = 'case%02d' % n
        names.append(name)
        # the restatement must agree before anything is stored: the randint calls (the round structure), the counts, coord, occupancy,
        # pixels exactly; ray_d / near / far bit for bit, or within the largest ulp distance found, which is recorded
        lens = [len(c) for c in sc['coords']]
        calls = []
        for n_body, n_face, n_rnd, kept in rounds:
            calls += [(lens[0], n_body)] + ([(lens[1], n_face)] if n_face >= 0 else []) + [(lens[2], n_rnd)]
        assert calls == r['calls'], (name, calls, r['calls'])
        assert sum(k for _, _, _, k in rounds) == len(r['near']) == len(mine['sel']) >= n_rand, name
        assert r['coord'].shape == mine['coord'].shape and np.array_equal(r['coord'], mine['coord']), name
        assert np.array_equal(r['occupancy'], mine['occupancy']) and r['occupancy'].dtype == np.uint8, name
        assert r['rgb'].dtype == np.float32 and r['rgb'].tobytes() == mine['rgb'].tobytes(), name
        assert r['mask_at_box'].all() and len(r['mask_at_box']) == len(r['near']) and np.array_equal(r['ray_o'], mine['ray_o']), name
        for k in ('ray_d', 'near', 'far'):
            assert r[k].dtype == np.float32 and r[k].shape == mine[k].shape, (name, k)
            max_ulp = max(max_ulp, S.ulp_distance(r[k], mine[k]))
        print(name, tag, want, 'seed', seed, 'N_rand', n_rand, 'ratios', body_ratio, face_ratio, 'rounds', rounds, 'n', len(r['near']),
              'max ulp so far', max_ulp)
        out[name + '_scene'] = np.array(tag)
        out[name + '_draw'] = np.array([seed, n_rand])
        out[name + '_ratios'] = np.array([body_ratio, face_ratio])
        out[name + '_rounds'] = np.array(rounds)
        out[name + '_coord'] = r['coord'].astype(np.int16)
        for k in ('occupancy', 'ray_d', 'near', 'far'):
            out[name + '_' + k] = r[k]
    out['cases'] = np.array(names)
    out['max_ulp'] = np.array(max_ulp)          # 0: the restatement's explicit sums equal this machine's np.dot bit for bit
    path = os.path.join(HERE, 'sample_small.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'max_ulp', max_ulp)
    assert os.path.getsize(path) < 300 * 1024


if __name__ == '__main__':
    main()
