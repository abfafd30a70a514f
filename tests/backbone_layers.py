"""The layer table of the backbone, shared by the tests that walk it (test infrastructure)."""


def backbone_layers(H, W):
    """(H, W, Cin, Cout, K, stride, dil) of every convolution behind the stem and the pooling (csrc/net.hip build_graph)."""
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    layers, inpl, cur_stride, cur_dil = [], 64, 4, 1
    for li, (nb, planes) in enumerate(zip((3, 4, 6, 3), (64, 128, 256, 512))):
        stride = 1 if li == 0 else 2
        down = stride != 1 or inpl != planes
        if down:
            if cur_stride == 8:
                cur_dil, stride = cur_dil * stride, 1
            else:
                cur_stride *= stride
        for bi in range(nb):
            s, cin = (stride if bi == 0 else 1), (inpl if bi == 0 else planes)
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            layers.append((h, w, cin, planes, 3, s, cur_dil))
            if bi == 0 and down:
                layers.append((h, w, cin, planes, 1, s, 1))
            layers.append((ho, wo, planes, planes, 3, 1, cur_dil))
            h, w = ho, wo
        inpl = planes
    layers.append((h, w, 512, 64, 1, 1, 1))
    return layers
