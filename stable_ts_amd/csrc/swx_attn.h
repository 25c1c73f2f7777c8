// swx_attn.h -- private to the three attention sources (swx_attn.hip, swx_xattn.hip, swx_selfattn.hip): all they share
#pragma once

constexpr int DH = 64;               // d_head of every Whisper size
