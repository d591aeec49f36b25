"""The two colour tables of the renderer, as data.

Provenance: matplotlib 3.10.8, ``matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3]`` for ``name`` in ("Blues", "turbo"): the
256 RGB entries ``imshow(cmap=name)`` indexes.  ``Blues`` is ColorBrewer's sequential scheme (Cynthia Brewer, colorbrewer2.org, Apache-2.0),
interpolated to 256 entries as matplotlib does; ``turbo`` is Anton Mikhailov's table (Google, Apache-2.0).  tests/golden/colormaps.npz holds
the same bytes, and tests/test_render.py compares both with the live colormaps where matplotlib is installed.  Each string is 256 x 3 bytes in hex."""
import numpy as np

_BLUES = (
    "f7fbfff6fafef5f9fef4f9fef3f8fdf3f8fdf2f7fdf1f7fdf0f6fceff6fceff5fceef5fcedf4fbecf4fbecf3fbebf3fbeaf2fae9f2fae8f1fae8f1fae7f0f9e6"
    "f0f9e5eff9e4eff9e4eef8e3eef8e2edf8e1edf8e1ecf7e0ecf7dfebf7deebf7ddeaf6ddeaf6dce9f6dbe9f6dae8f5dae8f5d9e7f5d8e7f5d7e6f4d7e6f4d6e5"
    "f4d5e5f4d4e4f3d4e4f3d3e3f3d2e3f3d1e2f2d1e2f2d0e1f2cfe1f2cee0f1cee0f1cddff1ccdff1cbdef0cbdef0caddf0c9ddf0c8dcefc8dcefc7dbefc6dbef"
    "c5daeec4daeec3d9eec1d9edc0d8edbfd8ecbed7ecbcd7ebbbd6ebbad6eab9d5eab7d4eab6d4e9b5d3e9b4d3e8b2d2e8b1d2e7b0d1e7afd1e6add0e6acd0e6ab"
    "cfe5aacfe5a8cee4a7cee4a6cde3a5cde3a3cce3a2cbe2a1cbe2a0cae19ecae19dc9e09bc8e09ac7e098c7df97c6df95c5df93c4de92c3de90c2de8fc1dd8dc0"
    "dd8bc0dd8abfdc88bedc87bddc85bcdb83bbdb82badb80b9da7fb8da7db8d97bb7d97ab6d978b5d877b4d875b3d873b2d772b1d770b1d76fb0d66dafd66baed6"
    "6aadd569acd567abd466aad465aad363a9d362a8d261a7d260a6d15ea5d15da4d05ca3d05aa3cf59a2cf58a1ce57a0ce559fcd549ecd539dcc519ccc509bcb4f"
    "9bcb4e9aca4c99ca4b98c94a97c94896c84795c84694c74594c74393c64292c64191c54090c53f8fc43e8ec43d8dc33c8cc33b8bc23a8ac13989c13888c03787"
    "c03585bf3484bf3383be3282be3181bd3080bd2f7fbc2e7ebc2d7dbb2c7cbb2b7bba2a7ab92979b92878b82777b82676b72575b72474b62373b62272b52171b5"
    "2070b41f6fb31e6eb21e6db21d6cb11c6bb01b6aaf1a69ae1a68ae1967ad1866ac1765ab1764ab1663aa1562a91461a81360a7135fa7125ea6115da5105ca40f"
    "5ba30f5aa30e59a20d58a10c57a00c56a00b559f0a549e09539d08529c08519c08509a084f99084e97084c96084b94084a9208499108488f08478e08468c0845"
    "8b084489084388084286084185084083083f82083e80083d7e083c7d083b7b083a7a08397808387708377508367408357208347108336f08326e08316c08306b"
)
_TURBO = (
    "30123b31154232184a341b51351e5836215f37236538266c3929723a2c793b2f7f3c32853c358b3d37913e3a963f3d9c4040a14043a64145ab4148b0424bb543"
    "4eba4350be4353c24456c74458cb455bce455ed24560d64563d94666dd4668e0466be3466de64670e84673eb4675ed4678f0467af2467df4467ff64682f84584"
    "f94587fb4589fc448cfd438efd4291fe4193fe4096fe3f98fe3e9bfe3c9dfd3ba0fc39a2fc38a5fb36a8f934aaf833acf631aff52fb1f32db4f12bb6ef2ab9ed"
    "28bbeb26bde925c0e623c2e421c4e120c6df1ec9dc1dcbda1ccdd71bcfd41ad1d219d3cf18d5cc18d7ca17d9c717dac417dcc217debf18e0bd18e1ba19e3b81a"
    "e4b61be5b41de7b11ee8af20e9ac22eba924eca627eda329eea02cef9d2ff09a32f19735f39438f4913bf48d3ff58a42f68746f7834af8804df97c51f97955fa"
    "7659fb725dfb6f61fc6c65fc6869fd656dfd6271fd5f74fe5c78fe597cfe5680fe5384fe5087fe4d8bfe4b8efe4892fe4695fe4498fe429bfd409efd3ea1fc3d"
    "a4fc3ba6fb3aa9fb39acfa37aef937b1f836b3f835b6f735b9f534bbf434bef334c0f233c3f133c5ef33c8ee33caed33cdeb34cfea34d1e834d4e735d6e535d8"
    "e335dae236dde036dfde36e1dc37e3da37e5d838e7d738e8d538ead339ecd139edcf39efcd39f0cb3af2c83af3c63af4c43af6c23af7c039f8be39f9bc39f9ba"
    "38fab737fbb537fbb336fcb035fcae34fdab33fda932fda631fda330fea12ffe9e2efe9b2dfe982cfd952bfd9229fd8f28fd8c27fc8926fc8624fb8323fb8022"
    "fa7d20fa7a1ff9771ef8741cf7711bf76e1af66b18f56817f46516f36315f26014f15d13ef5a11ee5810ed550fec520eea500de94d0de84b0ce6490be5460ae3"
    "440ae24209e04008de3e08dd3c07db3a07d93806d73606d63405d43205d23005d02f04ce2d04cb2b03c92903c72803c52602c32402c02302be2102bb1f01b91e"
    "01b61c01b41b01b11901ae1801ac1601a91501a61401a31201a011019d10019a0e01970d01940c01910b018e0a018b09018708018407018106027d05027a0402"
)


def _table(text: str) -> np.ndarray:
    t = np.frombuffer(bytes.fromhex(text), dtype=np.uint8).reshape(256, 3)
    t.flags.writeable = False
    return t


BLUES = _table(_BLUES)        # (256, 3) uint8, the signed distance
TURBO = _table(_TURBO)        # (256, 3) uint8, temperature and speed
