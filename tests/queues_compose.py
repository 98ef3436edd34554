"""A frame of the integrator composed from the public stages ON QUEUES — shared by tests/test_queues_device.py and tools/integrator_rate.py.  Per bounce:
closest, resolve, scatter (or its materials form); the wanted shadow rays compacted with their light rows, throughput and pixel; any-hit; the surviving paths compacted
(rays, Halton index, pixel, throughput).  Radiance goes to the dense image by pixel index: a pixel appears at most once per queue, so every sum has two terms and is exact.

Two forms:
  host_counts=True    the two counts of a bounce are read by the host, once, and every tensor is sliced to its count: the stages run on exactly the live rows
  host_counts=False   no host read at all: the counts stay on the device and go to the next stage as count=; torch's element-wise ops run over the capacity and what the
                      tail holds is masked by arange(n) < count before it can reach the image

The pixel columns are zeros before anything is written to them and a compaction never writes past its count, so a tail row always holds a valid pixel: nothing outside
the image is indexed even where a masked (zero) term is added.  The no-host-read form sends the zero term of tail row i to pixel i instead (i < n, the number of pixels):
thousands of tail rows adding to ONE pixel would be as many atomic adds on one address (measured: a 1080p frame took 66 ms so, and 239 ms with 70 % of its rows in the tail)."""


def compose_queued(torch, r, ds, sample_index, dev, bounces=3, materials=False, host_counts=True, info=None):
    """-> the frame's radiance sample, torch (n, 3) float32.  info: a dict that receives 'counts' (the path queue's length after each bounce but the last, one-element
    device tensors) and, with materials, 'lobes' ((lobe codes of the rows of a bounce, the count of that bounce or None) per bounce)"""
    rays, hidx = r.primary_rays_device(sample_index=sample_index)
    n = rays.shape[0]
    f32, i32 = torch.float32, torch.int32
    thr = torch.ones((n, 4), device=dev)                                                  # 16-byte rows; the fourth component is carried along and never read
    pix = torch.arange(n, dtype=i32, device=dev)
    acc = torch.zeros((n, 3), device=dev)
    rows = torch.arange(n, dtype=i32, device=dev)
    ws = [torch.empty(ds.compact_workspace_bytes(n), dtype=torch.uint8, device=dev) for _ in range(2)]
    # ping-pong destinations of the path queue and the destinations of the shadow queue; index columns start as zeros
    index = torch.empty if host_counts else torch.zeros                                   # (a tail is only ever looked at without the host's counts)
    path_out = [[torch.empty((n, 8), device=dev), index(n, dtype=i32, device=dev), index(n, dtype=i32, device=dev), torch.empty((n, 4), device=dev)] for _ in range(2)]
    shadow_out = [torch.empty((n, 8), device=dev), torch.empty((n, 4), device=dev), torch.empty((n, 4), device=dev), index(n, dtype=i32, device=dev)]
    cnt = None                                                                            # the path queue's length on the device (None: every row, bounce 0)
    live = n                                                                              # rows the tensors hold (host_counts: the queue's length; else the capacity)
    if info is not None: info["counts"] = []; info["lobes"] = []
    for b in range(bounces):
        kw = {} if host_counts or cnt is None else {"count": cnt}
        valid = None if host_counts or cnt is None else rows < cnt                        # the no-host-read form's mask of the live rows
        hits = ds.intersect_closest_device(rays, **kw)
        surf = ds.resolve_hits_device(rays, hits, **kw)
        last = b + 1 == bounces
        if materials:
            shadow, light, nxt, lobes = ds.scatter_materials_device(rays, surf, hidx, b, bounces, next_rays=not last, **kw)
            lobe = lobes[:, 3].view(i32)
            if info is not None: info["lobes"].append((lobe, None if host_counts else cnt))
            emitted = torch.mul(thr[:, 0:3], lobes[:, 4:7])
            if valid is not None: emitted = torch.where(valid[:, None], emitted, torch.zeros((), device=dev))
            acc.index_add_(0, pix if valid is None else torch.where(valid, pix, rows), emitted)          # emission along the path (a row that is no surface adds zero)
            thr[:, 0:3].mul_(lobes[:, 0:3])
            wanted = light[:, 3] == 1.0
            goes_on = (lobe >= 1) & (lobe <= 4)
        else:
            shadow, light, nxt = ds.scatter_device(surf, hidx, b, next_rays=not last, **kw)
            goes_on = surf[:, 7].view(i32) == 1                                           # a miss ends the path
            thr[:, 0:3].mul_(surf[:, 8:11])                                               # :339
            wanted = goes_on & (light[:, 3] == 1.0)
        so = [t[:live] for t in shadow_out]
        (s_rays, s_light, s_thr, s_pix), s_cnt = ds.compact_rows_device(wanted, [shadow, light, thr, pix], count=kw.get("count"), out=so, workspace=ws[0])
        if not last:
            po = [t[:live] for t in path_out[b & 1]]
            (rays, hidx, pix, thr), cnt = ds.compact_rows_device(goes_on, [nxt, hidx, pix, thr], count=kw.get("count"), out=po, workspace=ws[1])
            if info is not None: info["counts"].append(cnt)
        if host_counts:
            s_live, p_live = torch.cat([s_cnt, cnt if not last else s_cnt]).tolist()      # the one host read of the bounce
            s_rays, s_light, s_thr, s_pix = s_rays[:s_live], s_light[:s_live], s_thr[:s_live], s_pix[:s_live]
            occluded = ds.intersect_any_device(s_rays)
            lit = occluded == 0
            if not last:
                live = p_live
                rays, hidx, pix, thr = rays[:live], hidx[:live], pix[:live], thr[:live]
        else:
            occluded = ds.intersect_any_device(s_rays, count=s_cnt)
            s_valid = rows < s_cnt
            lit = (occluded == 0) & s_valid
            s_pix = torch.where(s_valid, s_pix, rows)
        term = torch.where(lit[:, None], torch.mul(s_light[:, 0:3], s_thr[:, 0:3]), torch.zeros((), device=dev))   # :371-373
        acc.index_add_(0, s_pix, term)
    return acc
