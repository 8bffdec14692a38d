"""`CustomDataset` read from a latent cache (ctrlora_amd/latent_cache.py, scripts/tool_cache_latents.py): items carry the stored
posteriors of the target and the condition image instead of the pixels,

    item["jpg_moments"]   float32 [2C, h, w]   (mean | std) of the target's posterior, unscaled
    item["hint_moments"]  float32 [2C, h, w]   the same of the condition image
    item["txt"]           the prompt, or '' with probability drop_rate -- the rule and the numpy stream of CustomDataset

so no image is decoded and `ControlLDM.get_input` runs neither VAE encode.  The text encoder stays live.  The cache is checked
against root/prompt.json (record list and count) here and against the model's first stage where training starts
(`ctrlora_amd.latent_cache.check_model`)."""
import numpy as np
from torch.utils.data import Dataset

from ctrlora_amd import latent_cache
from datasets.custom_dataset import CustomDataset


class CachedLatentDataset(Dataset):
    def __init__(self, root: str, cache_dir: str, drop_rate: float = 0.0):
        self.root, self.cache_dir, self.drop_rate = root, cache_dir, drop_rate
        self.data = CustomDataset(root, drop_rate=drop_rate).data
        self.meta, self.target, self.hint = latent_cache.open_cache(cache_dir)
        latent_cache.check_records(self.meta, self.data)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        rec = self.data[idx]
        prompt = "" if np.random.rand() < self.drop_rate else rec["prompt"]
        return dict(jpg_moments=np.array(self.target[idx]), hint_moments=np.array(self.hint[idx]), txt=prompt)
