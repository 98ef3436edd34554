"""A frame of the integrator composed from the public stages on queues with the path state kept by the library — shared by tests/test_paths_device.py and
tools/integrator_rate.py.  It is queues_compose.compose_queued with host_counts=False in which every torch op between the stages is one of the four path-state calls:
reset_paths_device before bounce 0; per bounce closest, resolve, scatter (or its materials form), advance_paths_device (throughput, emission, the two keep masks), the
wanted shadow rays compacted with their light rows, throughput and pixel, any-hit, deposit_light_device, and the surviving paths compacted.  Every stage takes the queue's
length as count=: no host read, no arange, no where, no index_add_ — and no stage looks past the count, so what a tail holds never matters."""


def compose_fused(torch, r, ds, sample_index, dev, bounces=3, materials=False, info=None, radiance=None):
    """-> the frame's radiance sample, torch (n, 4) float32 (.rgb; the fourth component is never changed).  radiance: the image to deposit into — rows of zeros, as
    fold_sample_device(clear_sample=True) leaves them — or None for a fresh one.  info: a dict that receives 'counts' (the path queue's length after each bounce but the
    last, one-element device tensors) and, with materials, 'lobes' ((lobe codes of the rows of a bounce, the count of that bounce or None) per bounce) and 'lobe_rows'
    (the (n, 8) lobe rows of each bounce)"""
    rays, hidx = r.primary_rays_device(sample_index=sample_index)
    n = rays.shape[0]
    i32, u8 = torch.int32, torch.uint8
    thr, pix, rad = ds.reset_paths_device(n, radiance=radiance is None)
    if radiance is not None: rad = radiance
    ws = [torch.empty(ds.compact_workspace_bytes(n), dtype=u8, device=dev) for _ in range(2)]
    masks = (torch.empty(n, dtype=u8, device=dev), torch.empty(n, dtype=u8, device=dev))
    # ping-pong destinations of the path queue and the destinations of the shadow queue
    path_out = [[torch.empty((n, 8), device=dev), torch.empty(n, dtype=i32, device=dev), torch.empty(n, dtype=i32, device=dev), torch.empty((n, 4), device=dev)] for _ in range(2)]
    shadow_out = [torch.empty((n, 8), device=dev), torch.empty((n, 4), device=dev), torch.empty((n, 4), device=dev), torch.empty(n, dtype=i32, device=dev)]
    occluded = torch.empty(n, dtype=i32, device=dev)
    cnt = None                                                                            # the path queue's length on the device (None: every row, bounce 0)
    if info is not None: info["counts"] = []; info["lobes"] = []; info["lobe_rows"] = []
    for b in range(bounces):
        kw = {} if cnt is None else {"count": cnt}
        last = b + 1 == bounces
        hits = ds.intersect_closest_device(rays, **kw)
        surf = ds.resolve_hits_device(rays, hits, **kw)
        out = masks if not last else masks[:1]
        if materials:
            shadow, light, nxt, lobes = ds.scatter_materials_device(rays, surf, hidx, b, bounces, next_rays=not last, **kw)
            if info is not None: info["lobes"].append((lobes[:, 3].view(i32), cnt)); info["lobe_rows"].append(lobes)
            wanted, goes_on = ds.advance_paths_device(light, thr, pixel=pix, radiance=rad, lobes=lobes, keep_path=not last, out=out, **kw)
        else:
            shadow, light, nxt = ds.scatter_device(surf, hidx, b, next_rays=not last, **kw)
            wanted, goes_on = ds.advance_paths_device(light, thr, surfaces=surf, keep_path=not last, out=out, **kw)
        (s_rays, s_light, s_thr, s_pix), s_cnt = ds.compact_rows_device(wanted, [shadow, light, thr, pix], count=cnt, out=shadow_out, workspace=ws[0])
        if not last:
            (rays, hidx, pix, thr), cnt = ds.compact_rows_device(goes_on, [nxt, hidx, pix, thr], count=cnt, out=path_out[b & 1], workspace=ws[1])
            if info is not None: info["counts"].append(cnt)
        ds.intersect_any_device(s_rays, out=occluded, count=s_cnt)
        ds.deposit_light_device(occluded, s_light, s_thr, s_pix, rad, count=s_cnt)
    return rad
